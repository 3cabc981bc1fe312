"""lib/materials/.  A material's to_abi(rec) fills its DrMaterial; `general` says whether it needs the general shading
kernels (anything but a Lambertian matte does: dr_api.hip's `general`)."""
import numpy as np

from .. import _abi


class MatteMaterial:
    """materials/matte_material.dart:37-77 with constant textures."""

    kind = _abi.DR_MATERIAL_MATTE

    def __init__(self, Kd=(0.5, 0.5, 0.5), sigma=0.0):
        self.Kd = np.asarray(Kd, dtype=np.float32).reshape(3)
        self.sigma = float(sigma)

    @property
    def general(self):  # sigma != 0 is OrenNayar
        return float(self.sigma) != 0.0

    def to_abi(self, rec):
        rec.type = self.kind
        rec.kd[:] = [float(x) for x in self.Kd]
        rec.sigma = float(self.sigma)


class MirrorMaterial:
    """materials/mirror_material.dart:35-62 with a constant Kr: one SpecularReflection(Kr, FresnelNoOp) lobe."""

    kind = _abi.DR_MATERIAL_MIRROR
    general = True

    def __init__(self, Kr=(0.9, 0.9, 0.9)):
        self.Kr = np.asarray(Kr, dtype=np.float32).reshape(3)

    def to_abi(self, rec):
        rec.type = self.kind
        rec.kr[:] = [float(x) for x in self.Kr]


class GlassMaterial:
    """materials/glass_material.dart:41-85 with constant textures: SpecularReflection(Kr, FresnelDielectric(1, index))
    + SpecularTransmission(Kt, 1, index)."""

    kind = _abi.DR_MATERIAL_GLASS
    general = True

    def __init__(self, Kr=(1.0, 1.0, 1.0), Kt=(1.0, 1.0, 1.0), index=1.5):
        self.Kr = np.asarray(Kr, dtype=np.float32).reshape(3)
        self.Kt = np.asarray(Kt, dtype=np.float32).reshape(3)
        self.index = float(index)

    def to_abi(self, rec):
        rec.type = self.kind
        rec.kr[:] = [float(x) for x in self.Kr]
        rec.kt[:] = [float(x) for x in self.Kt]
        rec.index = self.index


class PlasticMaterial:
    """materials/plastic_material.dart:40-85 with constant textures: Lambertian(Kd) + Microfacet(Ks,
    FresnelDielectric(1.5, 1.0), Blinn(1 / roughness))."""

    kind = _abi.DR_MATERIAL_PLASTIC
    general = True

    def __init__(self, Kd=(0.25, 0.25, 0.25), Ks=(0.25, 0.25, 0.25), roughness=0.1):
        self.Kd = np.asarray(Kd, dtype=np.float32).reshape(3)
        self.Ks = np.asarray(Ks, dtype=np.float32).reshape(3)
        self.roughness = float(roughness)
        self.Kr, self.index = self.Ks, self.roughness  # the fields the C ABI / oracle carry them in

    def to_abi(self, rec):
        rec.type = self.kind
        rec.kd[:] = [float(x) for x in self.Kd]
        rec.kr[:] = [float(x) for x in self.Ks]
        rec.index = self.roughness
