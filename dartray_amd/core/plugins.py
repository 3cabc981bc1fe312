"""The plugin registry (lib/core/plugin.dart:23-180): the names the reference registers in RegisterStandardPlugins
(render_manager_interface.dart:37-157) for the path."""
from .accel import BVHAccel
from .cameras import EnvironmentCamera, OrthographicCamera, PerspectiveCamera
from .film import BoxFilter, GaussianFilter, ImageFilm, LanczosSincFilter, MitchellFilter, TriangleFilter
from .lights import DiffuseAreaLight
from .materials import MatteMaterial
from .renderer import (AmbientOcclusionIntegrator, DiffusePRTIntegrator, DirectLightingIntegrator, EmissionIntegrator, FeatureIntegrator, GlossyPRTIntegrator, MaterialIntegrator, PathIntegrator, SamplerRenderer,
                       UseProbesIntegrator, WhittedIntegrator)
from .samplers import (AdaptiveSampler, HaltonSampler, LinearPixelSampler, LowDiscrepancySampler, RandomPixelSampler, RandomSampler,
                       StratifiedSampler, TilePixelSampler)
from .shapes import TriangleMesh


class Plugin:
    _reg = {"accelerator": {}, "surfaceIntegrator": {}, "renderer": {}, "sampler": {}, "film": {}, "filter": {},
            "camera": {}, "material": {}, "shape": {}, "areaLight": {}, "volumeIntegrator": {}, "pixelSampler": {}}

    @classmethod
    def register(cls, kind, name, creator):
        cls._reg[kind][name] = creator

    @classmethod
    def get(cls, kind, name):
        return cls._reg[kind].get(name)


def RegisterStandardPlugins():
    Plugin.register("accelerator", "bvh", BVHAccel.Create)
    Plugin.register("surfaceIntegrator", "path", lambda ps=None: PathIntegrator((ps or {}).get("maxdepth", 5)))
    Plugin.register("surfaceIntegrator", "directlighting",
                    lambda ps=None: DirectLightingIntegrator(1 if (ps or {}).get("strategy", "all") == "one" else 0, (ps or {}).get("maxdepth", 5)))
    Plugin.register("surfaceIntegrator", "whitted", WhittedIntegrator.Create)
    Plugin.register("surfaceIntegrator", "ambientocclusion", AmbientOcclusionIntegrator.Create)
    Plugin.register("surfaceIntegrator", "feature", FeatureIntegrator.Create)
    Plugin.register("surfaceIntegrator", "material", MaterialIntegrator.Create)
    Plugin.register("surfaceIntegrator", "diffuseprt", DiffusePRTIntegrator.Create)
    Plugin.register("surfaceIntegrator", "glossyprt", GlossyPRTIntegrator.Create)
    Plugin.register("surfaceIntegrator", "useprobes", UseProbesIntegrator.Create)
    Plugin.register("volumeIntegrator", "emission", lambda ps=None: EmissionIntegrator((ps or {}).get("stepsize", 1.0)))
    Plugin.register("renderer", "sampler", SamplerRenderer)
    Plugin.register("sampler", "lowdiscrepancy", LowDiscrepancySampler)
    Plugin.register("sampler", "stratified", StratifiedSampler)
    Plugin.register("sampler", "adaptive", AdaptiveSampler)
    Plugin.register("sampler", "halton", HaltonSampler)
    Plugin.register("sampler", "random", RandomSampler)
    Plugin.register("film", "image", ImageFilm)
    Plugin.register("pixelSampler", "linear", lambda ps=None: LinearPixelSampler())
    Plugin.register("pixelSampler", "tile", lambda ps=None: TilePixelSampler((ps or {}).get("tilesize", 32), (ps or {}).get("random", True)))
    Plugin.register("pixelSampler", "random", lambda ps=None: RandomPixelSampler())
    Plugin.register("filter", "box", lambda ps=None: BoxFilter((ps or {}).get("xwidth", 0.5), (ps or {}).get("ywidth", 0.5)))
    Plugin.register("filter", "gaussian", lambda ps=None: GaussianFilter((ps or {}).get("xwidth", 2.0), (ps or {}).get("ywidth", 2.0),
                                                                           (ps or {}).get("alpha", 2.0)))
    Plugin.register("filter", "sinc", lambda ps=None: LanczosSincFilter((ps or {}).get("xwidth", 4.0), (ps or {}).get("ywidth", 4.0),
                                                                          (ps or {}).get("tau", 3.0)))
    Plugin.register("filter", "mitchell", lambda ps=None: MitchellFilter((ps or {}).get("B", 1.0 / 3.0), (ps or {}).get("C", 1.0 / 3.0),
                                                                           (ps or {}).get("xwidth", 2.0), (ps or {}).get("ywidth", 2.0)))
    Plugin.register("filter", "triangle", lambda ps=None: TriangleFilter((ps or {}).get("xwidth", 2.0), (ps or {}).get("ywidth", 2.0)))
    Plugin.register("camera", "perspective", PerspectiveCamera)
    Plugin.register("camera", "orthographic", OrthographicCamera)
    Plugin.register("camera", "environment", EnvironmentCamera)
    Plugin.register("material", "matte", MatteMaterial)
    Plugin.register("shape", "trianglemesh", TriangleMesh)
    Plugin.register("areaLight", "diffuse", DiffuseAreaLight)


RegisterStandardPlugins()
