"""lib/renderers/, lib/surface_integrators/ and lib/volume_integrators/."""
import ctypes as C

import numpy as np

from .. import _abi
from .samplers import AdaptiveSampler, HaltonSampler, RoundUpPow2


class PathIntegrator:
    """surface_integrators/path_integrator.dart:26-27,133-136."""

    def __init__(self, maxDepth=5):
        self.maxDepth = int(maxDepth)

    kind = _abi.DR_INTEGRATOR_PATH

    def requestSamples(self, sampler, scene):
        """(n1D, n2D): entries of the 1-D and 2-D slots requestSamples asks of the sampler, in request order (:124-131):
        SAMPLE_DEPTH = 3 x (light 1D+2D, lightNum 1D, bsdf 1D+2D, path 1D+2D)."""
        return [1] * 12, [1] * 9

    @property
    def li_draws_recorded(self):
        """Li draws from the renderer's serial RNG (beyond its third vertex): a replay of that stream has to record those draws."""
        return self.maxDepth >= 3


class DirectLightingIntegrator:
    """surface_integrators/direct_lighting_integrator.dart:23-28: strategy 'all' (UniformSampleAllLights, the default) or 'one'
    (UniformSampleOneLight with the integrator's own lightNum slot, :51-55,82-87)."""
    SAMPLE_ALL_UNIFORM = 0
    SAMPLE_ONE_UNIFORM = 1

    def __init__(self, strategy=0, maxDepth=5):
        if strategy not in (self.SAMPLE_ALL_UNIFORM, self.SAMPLE_ONE_UNIFORM):
            raise ValueError("DirectLightingIntegrator strategy must be SAMPLE_ALL_UNIFORM (0) or SAMPLE_ONE_UNIFORM (1)")
        self.strategy = strategy
        self.maxDepth = int(maxDepth)

    @property
    def kind(self):
        return _abi.DR_INTEGRATOR_DIRECT_ONE if self.strategy == self.SAMPLE_ONE_UNIFORM else _abi.DR_INTEGRATOR_DIRECT_ALL

    li_draws_recorded = False

    def requestSamples(self, sampler, scene):
        """(n1D, n2D) as for PathIntegrator (:70-87).  "one": light component, lightNum, BSDF component; light position, BSDF direction.
        "all": per light a light and a BSDF slot pair of sampler.roundSize(nSamples) entries."""
        if self.strategy == self.SAMPLE_ONE_UNIFORM:
            return [1] * 3, [1] * 2
        ns = [sampler.roundSize(L.nSamples) for L in scene.lights]
        return [n for k in ns for n in (k, k)], [n for k in ns for n in (k, k)]


class WhittedIntegrator:
    """surface_integrators/whitted_integrator.dart:23-80: Le, one light sample per light, SpecularReflect / SpecularTransmit while
    ray.depth + 1 < maxDepth.  On the device DR_INTEGRATOR_WHITTED (k_shade_whitted)."""

    def __init__(self, maxDepth=5):
        self.maxDepth = int(maxDepth)

    kind = _abi.DR_INTEGRATOR_WHITTED
    li_draws_recorded = False  # (LightSample.random draws are keyed (pixel, sample) streams in every sampler mode)

    def requestSamples(self, sampler, scene):
        """No requestSamples in the reference: no slots of its own."""
        return [], []

    def check_sampler(self, sampler):
        """SamplerRenderer.describe: what this integrator asks of the renderer's sampler."""
        if getattr(sampler, "sampler_mode", None) == _abi.DR_SAMPLER_HOST_BUFFER and sampler.li_seed is None:
            raise ValueError("a WhittedIntegrator draws from the keyed (pixel, sample) streams in every sampler mode: give the "
                             "HostBufferSampler the seed of the render it replays (seed=...)")

    @staticmethod
    def Create(params=None):
        """WhittedIntegrator.Create (whitted_integrator.dart:74-77): `maxdepth`, default 5."""
        return WhittedIntegrator((params or {}).get("maxdepth", 5))


class AmbientOcclusionIntegrator:
    """surface_integrators/ambient_occlusion_integrator.dart:23-65: nSamples = RoundUpPow2(ns) occlusion rays Ray(p, w, minDist, maxDist) over the
    hemisphere of the camera hit's geometric normal, Li = nClear / nSamples.  On the device DR_INTEGRATOR_AO (k_shade_ao)."""

    def __init__(self, nSamples=2048, minDist=1.0e-4, maxDist=float("inf")):
        if int(nSamples) < 1:
            raise ValueError("ambient occlusion integrator: nsamples must be at least 1")
        self.nSamples = RoundUpPow2(int(nSamples))                 # :24-26
        if self.nSamples > 4096:
            raise ValueError("ambient occlusion integrator: nsamples above 4096 after rounding up to a power of two (the samplers' cap)")
        self.minDist, self.maxDist = float(minDist), float(maxDist)
        if not self.minDist >= 0.0:
            raise ValueError("ambient occlusion integrator: mindist must not be negative")
        if not self.maxDist > self.minDist:
            raise ValueError("ambient occlusion integrator: maxdist must be greater than mindist")

    kind = _abi.DR_INTEGRATOR_AO
    maxDepth = 1  # (not read by the device under this integrator; SamplerRenderer.describe marshals every integrator's)
    li_draws_recorded = False  # (the scramble's two randomUint() are keyed (pixel, sample) draws in every sampler mode)

    def requestSamples(self, sampler, scene):
        """No requestSamples in the reference: no slots of its own."""
        return [], []

    def check_sampler(self, sampler):
        """SamplerRenderer.describe: what this integrator asks of the renderer's sampler."""
        if isinstance(sampler, AdaptiveSampler):
            raise ValueError("ambient occlusion integrator: the adaptive sampler is not supported (its second pass over the rounds of "
                             "occlusion rays has no test; every other sampler mode is)")
        if getattr(sampler, "sampler_mode", None) == _abi.DR_SAMPLER_HOST_BUFFER and sampler.li_seed is None:
            raise ValueError("an AmbientOcclusionIntegrator draws its scramble from the keyed (pixel, sample) streams in every sampler mode: "
                             "give the HostBufferSampler the seed of the render it replays (seed=...)")

    def to_abi(self, d):
        """SamplerRenderer.describe, behind the sampler's own fields: the three parameters (they share storage with the tail pointers, which
        this integrator does not read: include/dartray_hip.h)."""
        d.ao_nsamples = self.nSamples
        d.ao_mindist = self.minDist
        d.ao_maxdist = self.maxDist

    @staticmethod
    def Create(params=None):
        """AmbientOcclusionIntegrator.Create (:55-60): `nsamples` 2048, `maxdist` infinity, `mindist` 1e-4."""
        ps = params or {}
        return AmbientOcclusionIntegrator(ps.get("nsamples", 2048), ps.get("mindist", 1.0e-4), ps.get("maxdist", float("inf")))


class DiffusePRTIntegrator:
    """surface_integrators/diffuse_prt_integrator.dart:23-92: the lights' direct radiance at the centre of the world bound projected onto
    (lmax + 1)^2 spherical harmonics once (preprocess), the cosine-weighted visibility of every camera hit projected onto the same basis with
    nSamples = RoundUpPow2(ns) occlusion rays, Li = Le + Kd * clamp(their dot product).  On the device DR_INTEGRATOR_DIFFUSE_PRT (k_shade_prt,
    dr_prt_project.hip).  Materials: matte with sigma 0; a scene with any other is refused by name at render time."""

    LMAX_MAX = 8

    def __init__(self, lmax=4, nSamples=4096):
        self.lmax = int(lmax)
        if self.lmax < 1:
            raise ValueError("diffuse PRT: lmax must be at least 1 (the Legendre recurrence stores P(1, 0) unconditionally)")
        if self.lmax > self.LMAX_MAX:
            raise ValueError("diffuse PRT: lmax above 8 (a camera sample's transfer coefficients, (lmax + 1)^2 words, live in a per-slot side buffer)")
        if int(nSamples) < 1:
            raise ValueError("diffuse PRT: nsamples must be at least 1")
        self.nSamples = RoundUpPow2(int(nSamples))                 # :26
        if self.nSamples > 4096:
            raise ValueError("diffuse PRT: nsamples above 4096 after rounding up to a power of two (the samplers' cap)")

    kind = _abi.DR_INTEGRATOR_DIFFUSE_PRT
    maxDepth = 1  # (not read by the device under this integrator; SamplerRenderer.describe marshals every integrator's)
    li_draws_recorded = False  # (the scramble's two randomUint() are keyed (pixel, sample) draws in every sampler mode)

    def requestSamples(self, sampler, scene):
        """The reference's requestSamples is empty (:42-43): no slots of its own."""
        return [], []

    def check_sampler(self, sampler):
        """SamplerRenderer.describe: what this integrator asks of the renderer's sampler."""
        if isinstance(sampler, AdaptiveSampler):
            raise ValueError("diffuse PRT: the adaptive sampler is not supported (its second pass over the rounds of occlusion rays has no "
                             "test; every other sampler mode is)")
        if getattr(sampler, "sampler_mode", None) == _abi.DR_SAMPLER_HOST_BUFFER and sampler.li_seed is None:
            raise ValueError("a DiffusePRTIntegrator draws its scramble from the keyed (pixel, sample) streams in every sampler mode: "
                             "give the HostBufferSampler the seed of the render it replays (seed=...)")

    def to_abi(self, d):
        """SamplerRenderer.describe, behind the sampler's own fields: the two parameters (union members at the offsets of ao_nsamples and
        feature_channel, which only their own integrators read: include/dartray_hip.h)."""
        d.prt_nsamples = self.nSamples
        d.prt_lmax = self.lmax

    def incident(self, scene, shutterOpen=0.0):
        """preprocess (:33-40) on the device: c_in after ReduceRinging, [(lmax + 1)^2, 3] f32 (dr_prt_incident)."""
        out = np.zeros(((self.lmax + 1) ** 2, 3), np.float32)
        _abi.check(_abi.lib().dr_prt_incident(scene._device().handle, self.lmax, float(shutterOpen), out.ctypes.data))
        return out

    @staticmethod
    def Create(params=None):
        """DiffusePRTIntegrator.Create (:83-87): `lmax` 4, `nsamples` 4096."""
        ps = params or {}
        return DiffusePRTIntegrator(ps.get("lmax", 4), ps.get("nsamples", 4096))


class GlossyPRTIntegrator:
    """surface_integrators/glossy_prt_integrator.dart:23-134: the incident light c_in as DiffusePRTIntegrator projects it and the BSDF matrix B of
    Lambertian(Kd) + Microfacet(Ks, FresnelDielectric(1.5, 1), Blinn(1 / roughness)) once (preprocess); at every camera hit the transfer matrix T
    from nSamples = RoundUpPow2(ns) occlusion rays, Li = Le + clamp(sum_i (B . Rotate(T . c_in))[i] * Ylm_i(woLocal)).  On the device
    DR_INTEGRATOR_GLOSSY_PRT (k_shade_gprt, k_gprt_finish, dr_prt_project.hip).  It reads no material function: every material
    the device path has is accepted."""

    LMAX_MAX = 4

    def __init__(self, Kd=0.5, Ks=0.25, roughness=0.1, lmax=4, nSamples=4096):
        rgb = lambda v: tuple(float(x) for x in (v if np.ndim(v) else (v, v, v)))
        self.Kd, self.Ks, self.roughness = rgb(Kd), rgb(Ks), float(roughness)
        self.lmax = int(lmax)
        if self.lmax < 1:
            raise ValueError("glossy PRT: lmax must be at least 1 (the Legendre recurrence stores P(1, 0) unconditionally)")
        if self.lmax > self.LMAX_MAX:
            raise ValueError("glossy PRT: lmax above 4 (the x-rotation rows are restated band by band, and a wave's registers hold the 325 "
                             "distinct elements of a transfer matrix at lmax 4)")
        if int(nSamples) < 1:
            raise ValueError("glossy PRT: nsamples must be at least 1")
        self.nSamples = RoundUpPow2(int(nSamples))                 # :25
        if self.nSamples > 4096:
            raise ValueError("glossy PRT: nsamples above 4096 after rounding up to a power of two (the samplers' cap)")

    kind = _abi.DR_INTEGRATOR_GLOSSY_PRT
    maxDepth = 1  # (not read by the device under this integrator; SamplerRenderer.describe marshals every integrator's)
    li_draws_recorded = False  # (the scramble's two randomUint() are keyed (pixel, sample) draws in every sampler mode)

    def requestSamples(self, sampler, scene):
        """The reference's requestSamples is empty (:53-54): no slots of its own."""
        return [], []

    def check_sampler(self, sampler):
        """SamplerRenderer.describe: what this integrator asks of the renderer's sampler."""
        if isinstance(sampler, AdaptiveSampler):
            raise ValueError("glossy PRT: the adaptive sampler is not supported (its second pass over the rounds of occlusion rays has no "
                             "test; every other sampler mode is)")
        if getattr(sampler, "sampler_mode", None) == _abi.DR_SAMPLER_HOST_BUFFER and sampler.li_seed is None:
            raise ValueError("a GlossyPRTIntegrator draws its scramble from the keyed (pixel, sample) streams in every sampler mode: "
                             "give the HostBufferSampler the seed of the render it replays (seed=...)")

    def to_abi(self, d):
        """SamplerRenderer.describe: the two parameters that travel in the descriptor (the union members diffuse PRT uses, read under this
        integrator's constant); Kd, Ks and roughness are set on the scene (bind)."""
        d.prt_nsamples = self.nSamples
        d.prt_lmax = self.lmax

    def bind(self, scene):
        """Sets Kd, Ks, roughness on the device scene (dr_scene_set_glossy_prt), where the BSDF matrix is cached per parameter set."""
        p = _abi.DrGlossyPrtParams((C.c_float * 3)(*self.Kd), (C.c_float * 3)(*self.Ks), self.roughness)
        _abi.check(_abi.lib().dr_scene_set_glossy_prt(scene._device().handle, C.byref(p)))

    def incident(self, scene, shutterOpen=0.0):
        """preprocess (:27-44) on the device: c_in after ReduceRinging, [(lmax + 1)^2, 3] f32 (dr_prt_incident)."""
        out = np.zeros(((self.lmax + 1) ** 2, 3), np.float32)
        _abi.check(_abi.lib().dr_prt_incident(scene._device().handle, self.lmax, float(shutterOpen), out.ctypes.data))
        return out

    def bsdf_matrix(self, scene, nsamples_b=1024):
        """preprocess (:46-48) on the device: B, [(lmax + 1)^2, (lmax + 1)^2, 3] f32 (dr_prt_bsdf_matrix); a render uses nsamples_b = 1024."""
        self.bind(scene)
        t = (self.lmax + 1) ** 2
        out = np.zeros((t, t, 3), np.float32)
        _abi.check(_abi.lib().dr_prt_bsdf_matrix(scene._device().handle, self.lmax, int(nsamples_b), out.ctypes.data))
        return out

    @staticmethod
    def Create(params=None):
        """GlossyPRTIntegrator.Create (:118-125): `Kd` 0.5, `Ks` 0.25, `roughness` 0.1, `lmax` 4, `nsamples` 4096."""
        ps = params or {}
        return GlossyPRTIntegrator(ps.get("Kd", 0.5), ps.get("Ks", 0.25), ps.get("roughness", 0.1), ps.get("lmax", 4), ps.get("nsamples", 4096))


class ProbeGrid:
    """A grid of radiance probes in the reference's Float32List form (create_probes_renderer.dart:139-160): lmax, includeDirect, includeIndirect,
    nProbes[3], the six bounds, the coefficients [cell][(lmax + 1)^2][3], three zeros.  `save` / `load`: the text form the reference's ReadFloatFile
    parses (common.dart:188-236) -- numbers of digits, '.', 'e', '-', '+' between white space, '#' comments -- every value with the nine
    significant digits that give a float32 back bit for bit."""

    def __init__(self, data):
        self.data = np.ascontiguousarray(data, np.float32).reshape(-1)
        if len(self.data) < 15:
            raise ValueError("a probe grid has at least 15 floats")

    lmax = property(lambda self: int(self.data[0]))
    includeDirect = property(lambda self: int(self.data[1]))
    includeIndirect = property(lambda self: int(self.data[2]))
    nProbes = property(lambda self: tuple(int(v) for v in self.data[3:6]))
    bounds = property(lambda self: self.data[6:12].copy())

    @property
    def coefficients(self):
        """[cells, (lmax + 1)^2, 3] f32, cell = x + y * nProbes[0] + z * nProbes[0] * nProbes[1]."""
        return self.data[12:-3].reshape(-1, (self.lmax + 1) ** 2, 3)

    def save(self, path):
        if not np.isfinite(self.data).all():
            raise ValueError("a probe grid with a value that is not finite has no text form (ReadFloatFile reads digits, '.', 'e', '-', '+')")
        with open(path, "w") as f:
            f.write("# radiance probes: lmax includeDirect includeIndirect nProbes[3] bounds[6] coefficients zeros[3]\n")
            for i in range(0, len(self.data), 6):
                f.write(" ".join("%.9g" % float(v) for v in self.data[i:i + 6]) + "\n")   # (the last number needs the newline: ReadFloatFile drops one that ends the text)

    @staticmethod
    def load(path):
        vals = []
        with open(path) as f:
            for line in f:
                vals.extend(float(t) for t in line.split("#", 1)[0].split())
        return ProbeGrid(np.array(vals, np.float64).astype(np.float32))


class UseProbesIntegrator:
    """surface_integrators/use_probes_integrator.dart:23-185: Li = Le + rho * INV_PI * clamp(E(n)), E the irradiance function of a grid of radiance
    probes -- interpolated trilinearly at the hit, convolved with the clamped cosine, evaluated at the shading normal facing the camera ray.  On the
    device DR_INTEGRATOR_USE_PROBES (k_shade_probes).  `probes`: a ProbeGrid (SamplerRenderer.create_probes bakes one), a float
    array in its form, or a file name.  Materials: matte with sigma 0; a grid baked without direct light is refused by name at render time."""

    def __init__(self, probes=None):
        if isinstance(probes, str):
            try:
                probes = ProbeGrid.load(probes)
            except (OSError, ValueError) as e:
                raise ValueError("use probes: cannot read the probe file %r (the `filename` parameter, default \"probes.out\": bake one with "
                                 "SamplerRenderer.create_probes(scene).save(filename)): %s" % (probes, e)) from e
        self.probes = probes if isinstance(probes, ProbeGrid) or probes is None else ProbeGrid(probes)

    kind = _abi.DR_INTEGRATOR_USE_PROBES
    maxDepth = 1  # (not read by the device under this integrator; SamplerRenderer.describe marshals every integrator's)
    li_draws_recorded = False  # (Li draws nothing that feeds its result: rho2's jitter is skipped for Lambertian lobes)
    bind_for_dumps = True  # (generate_samples / generate_halton_samples plan like a render: the plan refuses a scene without a grid)

    def requestSamples(self, sampler, scene):
        """:74-88: a light and a BSDF slot pair of sampler.roundSize(nSamples) entries per light -- DirectLighting "all"'s -- although Li reads none."""
        ns = [sampler.roundSize(L.nSamples) for L in scene.lights]
        return [n for k in ns for n in (k, k)], [n for k in ns for n in (k, k)]

    def check_sampler(self, sampler):
        """SamplerRenderer.describe: what this integrator asks of the renderer's sampler."""
        if isinstance(sampler, AdaptiveSampler):
            raise ValueError("use probes: the adaptive sampler is not supported (its second pass has no test under this integrator; every other "
                             "sampler mode is)")

    def bind(self, scene):
        """Attaches the grid to the device scene (dr_scene_set_probes); none: detaches whatever an earlier integrator attached."""
        h = scene._device().handle
        if self.probes is None:
            _abi.check(_abi.lib().dr_scene_set_probes(h, None, 0))
        else:
            _abi.check(_abi.lib().dr_scene_set_probes(h, self.probes.data.ctypes.data, len(self.probes.data)))

    @staticmethod
    def Create(params=None):
        """UseProbesIntegrator.Create (:172-175): `filename` "probes.out"."""
        return UseProbesIntegrator((params or {}).get("filename", "probes.out"))


class FeatureIntegrator:
    """The first-hit feature integrator (DR_INTEGRATOR_FEATURE, k_shade_feature; the reference has no such class): Li is one
    quantity of the camera ray's Intersection -- `channel` "ng" / "ns" (0.5 * (normal + 1), geometric / shading), "depth" (t, t, t), "uv"
    (u, v, 0) or "id" (primitive + 1, material + 1, 1) -- and 0 where the ray hits nothing.  No light is read."""

    CHANNELS = {"ng": _abi.DR_FEATURE_NG, "ns": _abi.DR_FEATURE_NS, "depth": _abi.DR_FEATURE_DEPTH, "uv": _abi.DR_FEATURE_UV,
                "id": _abi.DR_FEATURE_ID}

    def __init__(self, channel="ng"):
        if channel not in self.CHANNELS:
            raise ValueError("feature integrator: channel must be one of ng, ns, depth, uv, id (got %r)" % (channel,))
        self.channel = channel

    kind = _abi.DR_INTEGRATOR_FEATURE
    maxDepth = 0  # (not read by the device under this integrator; SamplerRenderer.describe marshals every integrator's)
    li_draws_recorded = False  # (Li draws nothing: a host-buffer replay needs neither tail nor seed)

    def requestSamples(self, sampler, scene):
        """No slots of its own."""
        return [], []

    def check_sampler(self, sampler):
        """SamplerRenderer.describe: what this integrator asks of the renderer's sampler."""
        if isinstance(sampler, AdaptiveSampler):
            raise ValueError("feature integrator: the adaptive sampler is not supported")

    def to_abi(self, d):
        """SamplerRenderer.describe, behind the sampler's own fields: the channel (the padding behind max_tail: include/dartray_hip.h)."""
        d.feature_channel = self.CHANNELS[self.channel]

    @staticmethod
    def Create(params=None):
        """`string channel`: ng (the default), ns, depth, uv or id."""
        return FeatureIntegrator((params or {}).get("channel", "ng"))


class MaterialIntegrator:
    """The first-hit material integrator (DR_INTEGRATOR_MATERIAL, k_shade_material; the reference has no such class), the
    feature integrator's sibling for what reads a material or a light: Li is, by `channel`, "albedo" -- the camera hit's material colour, Kd of
    matte and plastic, Kr of mirror and glass, 0 where the ray hits nothing -- or "emission" -- what Li of the Path, DirectLighting and Whitted
    integrators adds for the camera ray itself: isect.Le(-ray.d) at a hit, the lights' Le(ray) at a miss."""

    CHANNELS = {"albedo": _abi.DR_MATERIAL_CHANNEL_ALBEDO, "emission": _abi.DR_MATERIAL_CHANNEL_EMISSION}

    def __init__(self, channel="albedo"):
        if channel not in self.CHANNELS:
            raise ValueError("material integrator: channel must be one of albedo, emission (got %r)" % (channel,))
        self.channel = channel

    kind = _abi.DR_INTEGRATOR_MATERIAL
    maxDepth = 0  # (not read by the device under this integrator; SamplerRenderer.describe marshals every integrator's)
    li_draws_recorded = False  # (Li draws nothing: a host-buffer replay needs neither tail nor seed)

    def requestSamples(self, sampler, scene):
        """No slots of its own."""
        return [], []

    def check_sampler(self, sampler):
        """SamplerRenderer.describe: what this integrator asks of the renderer's sampler."""
        if isinstance(sampler, AdaptiveSampler):
            raise ValueError("material integrator: the adaptive sampler is not supported")

    def to_abi(self, d):
        """SamplerRenderer.describe, behind the sampler's own fields: the channel (a member of feature_channel's union: include/dartray_hip.h)."""
        d.material_channel = self.CHANNELS[self.channel]

    @staticmethod
    def Create(params=None):
        """`string channel`: albedo (the default) or emission."""
        return MaterialIntegrator((params or {}).get("channel", "albedo"))


class EmissionIntegrator:
    """volume_integrators/emission_integrator.dart with no VolumeRegion: T = 1,
    Lv = 0; its only effect on the path is the two 1-D sample slots it requests."""

    def __init__(self, stepSize=1.0):
        self.stepSize = stepSize


class OutputImage:
    """core/output_image.dart:35-55."""

    def __init__(self, xOffset, yOffset, width, height, rgb, film=None):
        self.xOffset, self.yOffset, self.width, self.height = xOffset, yOffset, width, height
        self.imageWidth, self.imageHeight = width, height
        self.rgb = rgb
        self.film = film  # (X, Y, Z, weightSum) per pixel: ImageFilm._Lxyz/_weightSum


class SamplerRenderer:
    """renderers/sampler_renderer.dart:28-31: Renderer.render(Scene) -> OutputImage."""

    def __init__(self, sampler, camera, surfaceIntegrator, volumeIntegrator=None, taskNum=0, taskCount=1,
                 tileRank=0, tileCount=1, tileSize=32):
        self.sampler = sampler
        self.camera = camera
        self.surfaceIntegrator = surfaceIntegrator
        self.volumeIntegrator = volumeIntegrator
        self.taskNum, self.taskCount = int(taskNum), int(taskCount)
        self.tileRank, self.tileCount, self.tileSize = int(tileRank), int(tileCount), int(tileSize)
        self.last_stats = None

    def requestSamples(self, sampler, scene):
        """(n1D, n2D): the surface integrator's slots, then the volume integrator's two 1-D ones -- tau and scatter, which the device's
        sample vector always carries (emission_integrator.dart:26-29)."""
        n1D, n2D = self.surfaceIntegrator.requestSamples(sampler, scene)
        return n1D + [1, 1], n2D

    def describe(self):
        """DrRenderDesc for this renderer (plus the arrays it points into)."""
        d = _abi.DrRenderDesc()
        self.camera.to_abi(d.camera)
        self.camera.film.to_abi(d.film)
        d.integrator = self.surfaceIntegrator.kind
        check = getattr(self.surfaceIntegrator, "check_sampler", None)
        if check:
            check(self.sampler)
        d.max_depth = self.surfaceIntegrator.maxDepth
        d.task_num, d.task_count = self.taskNum, self.taskCount
        d.tile_rank, d.tile_count, d.tile_size = self.tileRank, self.tileCount, self.tileSize
        keep = self.sampler.to_abi(d)
        fields = getattr(self.surfaceIntegrator, "to_abi", None)  # an integrator with parameters beyond maxDepth, behind the sampler's fields
        if fields:
            fields(d)
        return d, keep

    def generate_samples(self, scene, pixels):
        """dr_generate_samples: the device sampler's vectors for the raster pixels `pixels` ([n, 2]) -> [n * spp, nFloats] f32
        (AdaptiveSampler: the first pass's, spp = minSamples)."""
        if getattr(self.surfaceIntegrator, "bind_for_dumps", False):  # (the dump plans like a render, and UseProbesIntegrator's plan asks for the scene's grid)
            self.surfaceIntegrator.bind(scene)
        d, keep = self.describe()
        dev = scene._device()
        pixels = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
        nf = _abi.lib().dr_scene_sample_floats(dev.handle, d.integrator)
        out = np.zeros((len(pixels) * self.sampler.generatedSamplesPerPixel, nf), dtype=np.float32)
        _abi.check(_abi.lib().dr_generate_samples(dev.handle, C.byref(d), pixels.ctypes.data, len(pixels), out.ctypes.data, nf))
        return out

    def generate_halton_samples(self, scene, first=0, count=None):
        """dr_generate_halton_samples: the device sampler's accepted samples among the indices [first, first + count) of this task's
        sequence (count None: to its end) -> (k [n] uint64, pixel_xy [n, 2] int32, vectors [n, nFloats] f32), in increasing k."""
        if getattr(self.surfaceIntegrator, "bind_for_dumps", False):
            self.surfaceIntegrator.bind(scene)
        d, keep = self.describe()
        dev = scene._device()
        if count is None:
            _, _, w, h = HaltonSampler.window(self)
            count = (d.spp * max(w, h) ** 2 if w > 0 and h > 0 else 0) - first
        nf = _abi.lib().dr_scene_sample_floats(dev.handle, d.integrator)
        k = np.zeros(max(1, count), np.uint64)
        xy = np.zeros((max(1, count), 2), np.int32)
        out = np.zeros((max(1, count), nf), np.float32)
        n = C.c_uint64(0)
        _abi.check(_abi.lib().dr_generate_halton_samples(dev.handle, C.byref(d), first, count, k.ctypes.data, xy.ctypes.data, out.ctypes.data, nf, C.byref(n)))
        return k[:n.value].copy(), xy[:n.value].copy(), out[:n.value].copy()

    def prt_incident(self, scene):
        """The incident-light coefficients a DiffusePRTIntegrator render of `scene` uses (dr_prt_incident), [(lmax + 1)^2, 3] f32."""
        return self.surfaceIntegrator.incident(scene, self.camera.shutterOpen)

    def _probes_desc(self, lmax=4, spacing=1.0, bounds=None, time=0.0, npoints=32768, indirectlighting=False):
        d = _abi.DrProbesDesc()
        d.lmax, d.include_indirect, d.npoints, d.has_bounds = int(lmax), 1 if indirectlighting else 0, int(npoints), 0 if bounds is None else 1
        if bounds is not None:
            d.bounds[:] = [float(v) for v in np.asarray(bounds, np.float32).reshape(6)]
        # Point pCamera = camera.cameraToWorld.transformPoint(camera.shutterOpen, Point.ZERO) (:92-93): the translation column, a Point's f32
        d.camera_pos[:] = [float(np.float32(self.camera.cameraToWorld.reshape(4, 4)[k, 3])) for k in range(3)]
        d.spacing, d.time = float(spacing), float(time)
        return d

    def probes_surface_points(self, scene, npoints=32768, time=0.0):
        """Stage 1 of the bake (dr_probes_surface_points): the surface points the random walks from the camera deposit, [n, 3] f32."""
        d = self._probes_desc(npoints=npoints, time=time)
        out, n = np.zeros((int(npoints) + 32, 3), np.float32), C.c_int32(0)
        _abi.check(_abi.lib().dr_probes_surface_points(scene._device().handle, d.camera_pos, d.time, d.npoints, out.ctypes.data, C.byref(n)))
        return out[:n.value].copy()

    def probes_grid(self, scene, spacing=1.0, bounds=None):
        """(nProbes (3 ints), bounds [6] f32) of a bake with these parameters (dr_probes_grid)."""
        d, n, b = self._probes_desc(spacing=spacing, bounds=bounds), (C.c_int32 * 3)(), (C.c_float * 6)()
        _abi.check(_abi.lib().dr_probes_grid(scene._device().handle, C.byref(d), n, b))
        return tuple(n), np.array(b, np.float32)

    def probes_candidates(self, scene, points, spacing=1.0, bounds=None, time=0.0):
        """Stage 2 of the bake (dr_probes_candidates): (nFound [cells], accepted [cells, 32], -1 behind the last) for the given surface points."""
        d = self._probes_desc(spacing=spacing, bounds=bounds, time=time)
        n, _ = self.probes_grid(scene, spacing, bounds)
        cells = n[0] * n[1] * n[2]
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        nfound, acc = np.zeros(cells, np.int32), np.zeros((cells, 32), np.int32)
        _abi.check(_abi.lib().dr_probes_candidates(scene._device().handle, C.byref(d), pts.ctypes.data, len(pts), nfound.ctypes.data, acc.ctypes.data))
        return nfound, acc

    def create_probes(self, scene, lmax=4, spacing=1.0, bounds=None, time=0.0, npoints=32768, indirectlighting=False):
        """CreateProbesRenderer.render (renderers/create_probes_renderer.dart:51-168) on the device (dr_probes_bake): shadowed direct light
        projected onto (lmax + 1)^2 spherical harmonics at up to 32 visible points per cell of a grid over `bounds` (default: the scene's world
        bound), as a ProbeGrid.  indirectlighting defaults to FALSE here -- the reference's default is true -- because that half, a full render
        per probe direction, is not served: asking for it is refused by name."""
        d = self._probes_desc(lmax, spacing, bounds, time, npoints, indirectlighting)
        n, _ = self.probes_grid(scene, spacing, bounds)
        out = np.zeros(15 + n[0] * n[1] * n[2] * (int(lmax) + 1) ** 2 * 3, np.float32)
        _abi.check(_abi.lib().dr_probes_bake(scene._device().handle, C.byref(d), out.ctypes.data, len(out)))
        return ProbeGrid(out)

    def prt_bsdf_matrix(self, scene, nsamples_b=1024):
        """The BSDF matrix a GlossyPRTIntegrator render of `scene` uses (dr_prt_bsdf_matrix), [(lmax + 1)^2, (lmax + 1)^2, 3] f32."""
        return self.surfaceIntegrator.bsdf_matrix(scene, nsamples_b)

    def render(self, scene):
        film = self.camera.film
        if hasattr(self.surfaceIntegrator, "bind"):  # (an integrator with parameters that live on the scene: GlossyPRTIntegrator)
            self.surfaceIntegrator.bind(scene)
        d, keep = self.describe()
        out_film = np.zeros((film.height, film.width, 4), dtype=np.float32)
        out_rgb = np.zeros((film.height, film.width, 3), dtype=np.float32)
        dev = scene._device()
        dev.reset_stats()
        _abi.check(_abi.lib().dr_render(dev.handle, C.byref(d), out_film.ctypes.data, out_rgb.ctypes.data))
        del keep
        self.last_stats = dev.stats()
        return OutputImage(film.left, film.top, film.width, film.height, out_rgb, out_film)

    def guides_desc(self, scene, channels):
        """(DrRenderDesc, the arrays it points into, DrGuidesDesc) of render_with_guides(scene, channels), checked: the integrator's and the
        sampler's own rules (describe), then dr_render_guides_check, whose refusal raises ValueError with the library's text.  Needs no device."""
        channels = tuple(channels)
        unknown = [c for c in channels if c not in FeatureIntegrator.CHANNELS]
        if unknown:
            raise ValueError("render guides: channel must be one of ng, ns, depth, uv, id (got %r)" % (unknown[0],))
        d, keep = self.describe()
        g = _abi.DrGuidesDesc()
        g.count = len(channels)
        for i, c in enumerate(channels[:_abi.DR_GUIDES_MAX]):
            g.channels[i] = FeatureIntegrator.CHANNELS[c]
        lib = _abi.lib()
        if lib.dr_render_guides_check(C.byref(d), C.byref(g), len(scene.aggregate.tri_idx)) != _abi.DR_OK:
            raise ValueError("%s (surface integrator %s, sampler %s)" % (lib.dr_last_error().decode(), type(self.surfaceIntegrator).__name__,
                                                                       type(self.sampler).__name__))
        return d, keep, g

    def render_with_guides(self, scene, channels=("ns", "depth")):
        """render(), and in the same pass the FeatureIntegrator images of `channels` (dr_render_guides): the OutputImage of
        render() with `guides`, a dict channel -> [h, w, 3] f32, and `guide_films`, channel -> [h, w, 4], on it.  Each equals what a render
        of FeatureIntegrator(channel) with this renderer's camera, sampler and work split returns.  Path, DirectLighting, Whitted and
        ambient occlusion integrators; any other, and the adaptive sampler, raise ValueError before anything is rendered."""
        channels = tuple(channels)
        d, keep, g = self.guides_desc(scene, channels)
        film = self.camera.film
        out_film = np.zeros((film.height, film.width, 4), dtype=np.float32)
        out_rgb = np.zeros((film.height, film.width, 3), dtype=np.float32)
        films = [np.zeros((film.height, film.width, 4), dtype=np.float32) for _ in channels]
        rgbs = [np.zeros((film.height, film.width, 3), dtype=np.float32) for _ in channels]
        film_ptrs = (C.c_void_p * len(channels))(*[a.ctypes.data for a in films])
        rgb_ptrs = (C.c_void_p * len(channels))(*[a.ctypes.data for a in rgbs])
        dev = scene._device()
        dev.reset_stats()
        _abi.check(_abi.lib().dr_render_guides(dev.handle, C.byref(d), C.byref(g), out_film.ctypes.data, out_rgb.ctypes.data, film_ptrs, rgb_ptrs))
        del keep
        self.last_stats = dev.stats()
        out = OutputImage(film.left, film.top, film.width, film.height, out_rgb, out_film)
        out.guides = dict(zip(channels, rgbs))
        out.guide_films = dict(zip(channels, films))
        return out

    def supersampled_pixels(self, scene):
        """The raster pixels the last render of `scene` traced at maxSamples ([n, 2] int32, no particular order; AdaptiveSampler)."""
        return scene._device().adaptive_pixels()

    def render_sharded(self, scene, root=0):
        """One rank's part of a sharded render (dr_render_sharded): this renderer's tile / task share, ONE film reduce over
        the communicator of dr_comm_init, and on the root rank the OutputImage; other ranks return None.  What
        RenderManager's fan-out and rectangle merge do in the host (render_manager.dart:100-141), as one C call."""
        film = self.camera.film
        if hasattr(self.surfaceIntegrator, "bind"):
            self.surfaceIntegrator.bind(scene)
        d, keep = self.describe()
        lib = _abi.lib()
        is_root = lib.dr_comm_world() <= 1 or lib.dr_comm_rank() == root
        out_film = np.zeros((film.height, film.width, 4), dtype=np.float32) if is_root else None
        out_rgb = np.zeros((film.height, film.width, 3), dtype=np.float32) if is_root else None
        dev = scene._device()
        _abi.check(lib.dr_render_sharded(dev.handle, C.byref(d), root, out_film.ctypes.data if is_root else None,
                                         out_rgb.ctypes.data if is_root else None))
        del keep
        return OutputImage(film.left, film.top, film.width, film.height, out_rgb, out_film) if is_root else None

    def pixels(self):
        """Raster pixels this renderer's task / tile share traces, in trace order (host-only)."""
        d, keep = self.describe()
        n = C.c_uint64(0)
        _abi.check(_abi.lib().dr_enumerate_pixels(C.byref(d), None, 0, C.byref(n)))
        out = np.zeros((n.value, 2), dtype=np.int32)
        _abi.check(_abi.lib().dr_enumerate_pixels(C.byref(d), out.ctypes.data, n.value, C.byref(n)))
        return out

    def render_device(self, scene, film_ptr, stream=0):
        """Renderer.render with the film left in HBM: accumulates this renderer's share into the
        [height, width, 4] f32 device buffer at `film_ptr` on HIP stream `stream` (asynchronous)."""
        if hasattr(self.surfaceIntegrator, "bind"):
            self.surfaceIntegrator.bind(scene)
        d, keep = self.describe()
        dev = scene._device()
        _abi.check(_abi.lib().dr_render_device(dev.handle, C.byref(d), film_ptr, stream))
        self._keep = keep
        return dev

    def Li(self, *a, **k):  # a per-ray FFI seam is far too fine grained
        raise NotImplementedError("SamplerRenderer.Li is evaluated on the device inside render()")
