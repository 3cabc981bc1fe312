"""lib/lights/.  A light's to_abi(rec, ctx) fills its DrAreaLight; what it adds beside that record -- light triangles, an
environment map -- goes into ctx (LightContext).  `general` says whether the light needs the general shading kernels."""
import math

import numpy as np

from .. import _abi
from .transform import _inv, _normalize, transform_points


class LightContext:
    """What the lights of one Scene write beside their own records: light_tris grows by every area light's
    (v0, v1, v2, flags) rows, env_maps by every DrEnvMap; base_of / quad_of give a mesh's first vertex and a quadric's
    index in the aggregate, by id()."""

    def __init__(self, base_of, quad_of):
        self.light_tris, self.env_maps = [], []
        self.base_of, self.quad_of = base_of, quad_of


class PointLight:
    """lights/point_light.dart:35-47: an isotropic delta light at lightToWorld(0,0,0) with intensity I."""

    def __init__(self, light2world=None, I=(1.0, 1.0, 1.0)):
        m = np.eye(4, dtype=np.float32) if light2world is None else np.asarray(light2world, np.float32).reshape(4, 4)
        self.lightToWorld = m
        self.lightPos = transform_points(m, np.zeros((1, 3), np.float32))[0]
        self.intensity = np.asarray(I, dtype=np.float32).reshape(3)
        self.nSamples = 1
        self.shape = None

    abi_kind = _abi.DR_LIGHT_POINT
    general = True

    def isDeltaLight(self):
        return True

    def to_abi(self, rec, ctx):
        rec.L[:] = [float(x) for x in self.intensity]
        rec.nsamples = 1
        rec.kind = self.abi_kind
        rec.position[:] = [float(x) for x in self.lightPos]


class SpotLight(PointLight):
    """lights/spot_light.dart:40-85: a point light with a smooth-step cone about light-space +z; `width` and `fall`
    are the total cone angle and the falloff start, degrees."""

    def __init__(self, light2world=None, I=(1.0, 1.0, 1.0), width=30.0, fall=25.0, world2light=None):
        super().__init__(light2world, I)
        self.worldToLight = _inv(self.lightToWorld) if world2light is None else np.asarray(world2light, np.float32).reshape(4, 4)
        self.width, self.fall = float(width), float(fall)

    # True: marshal what a host that only holds the constructed SpotLight has (spot_light.dart:46-47): the two cosines
    marshal_cosines = False

    @property
    def abi_kind(self):
        return _abi.DR_LIGHT_SPOT_COS if self.marshal_cosines else _abi.DR_LIGHT_SPOT

    def to_abi(self, rec, ctx):
        super().to_abi(rec, ctx)
        rec.world_to_light[:] = [float(x) for x in self.worldToLight.reshape(-1)]
        if self.marshal_cosines:
            rec.cone_width = math.cos(math.radians(self.width))
            rec.cone_falloff_start = math.cos(math.radians(self.fall))
        else:
            rec.cone_width, rec.cone_falloff_start = self.width, self.fall


class DistantLight:
    """lights/distant_light.dart:37-61: radiance L arriving from direction lightDir = normalize(lightToWorld(dir))."""

    def __init__(self, light2world=None, L=(1.0, 1.0, 1.0), dir=(0.0, 0.0, -1.0)):
        m = np.eye(4, dtype=np.float32) if light2world is None else np.asarray(light2world, np.float32).reshape(4, 4)
        self.lightToWorld = m
        d = np.asarray(dir, np.float64).astype(np.float32).astype(np.float64)
        v = np.array([m[r, 0] * d[0] + m[r, 1] * d[1] + m[r, 2] * d[2] for r in range(3)], np.float64).astype(np.float32)
        self.lightDir = _normalize(v)
        self.lightPos = self.lightDir  # the field the C ABI / oracle carry it in
        self.intensity = np.asarray(L, dtype=np.float32).reshape(3)
        self.nSamples = 1
        self.shape = None

    abi_kind = _abi.DR_LIGHT_DISTANT
    general = True

    def isDeltaLight(self):
        return True

    to_abi = PointLight.to_abi  # (the direction travels in `position`)


def delta_light_kind(L):
    return L.abi_kind


class DiffuseAreaLight:
    """lights/diffuse_area_light.dart:36-43."""

    def __init__(self, L=(1.0, 1.0, 1.0), nSamples=1, shape=None):
        self.Lemit = np.asarray(L, dtype=np.float32).reshape(3)
        self.nSamples = max(1, int(nSamples))
        self.shape = shape

    general = False

    def to_abi(self, rec, ctx):
        """The light's ShapeSet (shape_set.dart:25-35) as rows of ctx.light_tris: an intersectable shape whole, a mesh's
        triangles in refine (reversed) order."""
        first = len(ctx.light_tris)
        ctx.light_tris += self.shape.light_rows(ctx)
        rec.L[:] = [float(x) for x in self.Lemit]
        rec.nsamples = self.nSamples
        rec.first_tri = first
        rec.ntris = len(ctx.light_tris) - first


class InfiniteAreaLight:
    """lights/infinite_area_light.dart:36-68.  `texels` is the radiance map's image [H, W, 3] f32 as MIPMap.texture receives it (a
    size that is no power of two is resampled up to the next one, mipmap.dart:71-138: dr_scene_create does that) -- None gives the
    1x1 white map of the no-'mapname' case;
    `L` the factor _radiance() multiplies in (:180-182).  NB when the reference loads a map from a file it
    ALSO pre-multiplies the texels by L (:44-49), i.e. L is applied twice; callers that want that pass
    pre-multiplied texels."""

    def __init__(self, light2world=None, L=(1.0, 1.0, 1.0), nSamples=1, texels=None):
        m = np.eye(4, dtype=np.float32) if light2world is None else np.asarray(light2world, np.float32).reshape(4, 4)
        self.lightToWorld = m
        self.worldToLight = _inv(m)  # Transform.Inverse (light.dart:30) of a Transform made from the matrix alone (transform.dart:31-35)
        self.L = np.asarray(L, dtype=np.float32).reshape(3)
        self.Lemit = self.L
        self.nSamples = max(1, int(nSamples))
        if texels is None:
            texels = np.ones((1, 1, 3), dtype=np.float32)
        self.texels = np.ascontiguousarray(texels, dtype=np.float32)
        self.shape = None

    general = False

    def isDeltaLight(self):
        return False

    def to_abi(self, rec, ctx):
        e = _abi.DrEnvMap()
        e.texels = self.texels.ctypes.data
        e.height, e.width = self.texels.shape[0], self.texels.shape[1]
        e.light_to_world[:] = [float(v) for v in self.lightToWorld.reshape(-1)]
        e.world_to_light[:] = [float(v) for v in self.worldToLight.reshape(-1)]
        rec.L[:] = [float(x) for x in self.L]
        rec.nsamples = self.nSamples
        rec.kind = _abi.DR_LIGHT_INFINITE
        rec.env_index = len(ctx.env_maps)
        ctx.env_maps.append(e)
