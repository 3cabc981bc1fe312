"""The first-hit material integrator on the GPU (DR_INTEGRATOR_MATERIAL, k_shade_material) against the Python restatement
(tests/material_restatement.py) fed the device sampler's own vectors, as tests/test_gpu_feature.py compares the feature integrator: 16 x 16
images at 2 samples per pixel over eleven primitives (tests/material_cases.py), box filter 0.5, so film and rgb are compared bit for bit.  A
restated film is computed once per (channel, background, sampler) and shared.  Nothing is started after a failed call: every call's return
code raises."""
import ctypes as C

import numpy as np
import pytest

from dartray_amd import _abi, core, scenes

import feature_restatement as fe
import material_cases as mc
import material_restatement as me

pytestmark = pytest.mark.gpu

SEED = 5489
CHANNELS = ["albedo", "emission"]


class Setup:
    """One aggregate under two light lists -- its area lights alone ("dark") and with an infinite light behind them ("sky") -- on both sides."""

    def __init__(self):
        self.accel = acc = core.BVHAccel(mc.yard_prims())
        self.lights = {"dark": acc.lights(), "sky": acc.lights() + [mc.sky()]}
        self.scene = {k: core.Scene(acc, v) for k, v in self.lights.items()}
        self.restated = {k: mc.restated(acc, v) for k, v in self.lights.items()}
        self.cache = {}

    def camera(self, filt=None):
        film = core.ImageFilm(16, 16, filt or core.BoxFilter(0.5, 0.5))
        return core.PerspectiveCamera.lookAt((0.0, 3.0, -6.0), (0.0, 1.2, 2.0), (0.0, 1.0, 0.0), 50.0, film)

    def renderer(self, channel, mk, cam=None, **kw):
        cam = cam or self.camera()
        return core.SamplerRenderer(mk(cam), cam, core.MaterialIntegrator(channel), core.EmissionIntegrator(), **kw)

    def restated_render(self, channel, bg, mk, key, filt=None):
        """(Ls, hit, film, rgb, pixels, vectors) of the restatement for the vectors the device sampler mk(camera) generates (cached)."""
        k = (channel, bg, key)
        if k not in self.cache:
            cam = self.camera(filt)
            r = self.renderer(channel, mk, cam)
            pixels = r.pixels()
            vec = r.generate_samples(self.scene[bg], pixels)
            spp = r.sampler.samplesPerPixel
            assert vec.shape == (len(pixels) * spp, 7)                 # image, lens, time, tau, scatter: no slots of its own
            rcam = fe.dr.PerspectiveCamera(cam.rasterToCamera.reshape(-1), cam.cameraToWorld.reshape(-1), cam.lensRadius, cam.focalDistance)
            f = cam.film
            self.cache[k] = me.render(self.restated[bg], me.CHANNELS[channel], rcam, f.xResolution, f.yResolution, f.filter.xWidth, f.filter.yWidth,
                                      f.filterTable, spp, pixels, vec) + (pixels, vec)
        return self.cache[k]


@pytest.fixture(scope="module")
def yard(gpu):
    return Setup()


def _ld(cam, spp=2):
    return core.LowDiscrepancySampler(cam, spp, SEED)


SAMPLERS = {
    "stratified": lambda cam: core.StratifiedSampler(cam, 2, 1, True, SEED),
    "stratified_nojitter": lambda cam: core.StratifiedSampler(cam, 2, 1, False, SEED),
    "random": lambda cam: core.RandomSampler(cam, 2, SEED),
}


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _with_option(name, value, fn):
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(name.encode(), str(value).encode()))
        return fn()
    finally:
        lib.dr_set_option(name.encode(), None)


# ---- 1. both channels, with and without an infinite light, against the restatement ----
@pytest.mark.parametrize("bg", ["dark", "sky"])
@pytest.mark.parametrize("channel", CHANNELS)
def test_both_channels_equal_the_restatement_bit_for_bit(yard, channel, bg):
    Ls, hit, film, rgb, pixels, vec = yard.restated_render(channel, bg, _ld, "counter")
    assert len(pixels) == 17 * 17 and 40 < hit.sum() < len(hit) - 40    # hits and misses both
    out = yard.renderer(channel, _ld).render(yard.scene[bg])
    assert np.isfinite(out.film).all() and _same(out.film, film) and _same(out.rgb, rgb)
    assert (Ls >= 0.0).all() and film[..., :3].max() > 0.0


def test_the_scene_is_what_the_cases_need(yard):
    """The restated samples themselves: every material kind gives its own colour; the emitters seen from the front give their Lemit and the
    disk seen from behind 0; a miss is black without the infinite light and its map's radiance with it, and the albedo of a miss is 0."""
    albedo, hit = yard.restated_render("albedo", "dark", _ld, "counter")[:2]
    colours = {tuple(c) for c in albedo[hit]}
    F = lambda *v: tuple(np.float32(x) for x in v)
    for c in (F(0.7, 0.6, 0.5), F(0.2, 0.3, 0.4), F(0.1, 0.8, 0.1), F(0.9, 0.85, 0.8), F(0.3, 0.2, 0.6), F(0.95, 0.9, 1.0), F(0.6, 0.1, 0.1), F(0.5, 0.5, 0.5)):
        assert c in colours, c                                           # matte x 3, mirror Kr, plastic Kd, glass Kr, the sphere, the emitters' own matte
    assert (albedo[~hit] == 0.0).all()
    dark, sky = (yard.restated_render("emission", bg, _ld, "counter")[0] for bg in ("dark", "sky"))
    lit = {tuple(c) for c in dark[hit]}
    assert lit == {F(0.0, 0.0, 0.0), F(5.0, 4.0, 3.0), F(1.0, 2.0, 9.0), F(8.0, 8.0, 2.0)}       # the back-facing disk's (2, 7, 1) is never seen
    assert (dark[~hit] == 0.0).all() and (sky[~hit] > 0.0).any() and len({tuple(c) for c in sky[~hit]}) > 20 and _same(dark[hit], sky[hit])


# ---- 2. the sampler modes ----
@pytest.mark.parametrize("name", sorted(SAMPLERS))
@pytest.mark.parametrize("channel", CHANNELS)
def test_other_pixel_bound_samplers_equal_the_restatement_fed_their_vectors(yard, channel, name):
    film, rgb = yard.restated_render(channel, "sky", SAMPLERS[name], name)[2:4]
    out = yard.renderer(channel, SAMPLERS[name]).render(yard.scene["sky"])
    assert _same(out.film, film) and _same(out.rgb, rgb)
    assert not _same(film, yard.restated_render(channel, "sky", _ld, "counter")[2])


@pytest.mark.parametrize("channel", CHANNELS)
def test_host_buffer_replay_equals_the_counter_film(yard, channel):
    Ls, hit, film, rgb, pixels, vec = yard.restated_render(channel, "sky", _ld, "counter")
    out = yard.renderer(channel, lambda cam: core.HostBufferSampler(cam, 2, pixels, vec)).render(yard.scene["sky"])
    assert _same(out.film, film) and _same(out.rgb, rgb)


@pytest.mark.parametrize("channel", CHANNELS)
def test_halton_sampler_equals_the_restatement(yard, channel):
    """The Halton sampler's samples belong to the image and its slots are single samples, which k_film adds by f32 atomics in no fixed order.
    A sum of one or two terms does not depend on the order, so every pixel that received at most two samples is compared bit for bit; a
    pixel with three or more at the splats' 2e-5 (tests/test_gpu_feature.py's Halton case).  The weights are counts and equal exactly."""
    cam = yard.camera()
    r = yard.renderer(channel, lambda c: core.HaltonSampler(c, 2, SEED), cam)
    k, xy, vec = r.generate_halton_samples(yard.scene["sky"])
    assert len(k) > 300 and vec.shape == (len(k), 7)
    rcam = fe.dr.PerspectiveCamera(cam.rasterToCamera.reshape(-1), cam.cameraToWorld.reshape(-1), cam.lensRadius, cam.focalDistance)
    Ls, hit, film, rgb = me.render(yard.restated["sky"], me.CHANNELS[channel], rcam, 16, 16, 0.5, 0.5, cam.film.filterTable, 1, xy, vec)
    out = r.render(yard.scene["sky"])
    assert np.array_equal(out.film[..., 3], film[..., 3])
    few = film[..., 3] <= 2.0
    print("halton %s: %d pixels with at most two samples, %d with more; max |device - restatement| = %.3g"
          % (channel, few.sum(), (~few).sum(), np.abs(out.film - film).max()))
    assert few.sum() > 100 and _same(out.film[few], film[few]) and _same(out.rgb[few], rgb[few])
    assert np.allclose(out.film, film, rtol=2e-5, atol=2e-6) and np.allclose(out.rgb, rgb, rtol=2e-5, atol=2e-6)


# ---- 3. state layouts; a wide filter ----
@pytest.mark.parametrize("layout", [64, 4])
@pytest.mark.parametrize("channel", CHANNELS)
def test_both_state_layouts_give_the_same_bytes(yard, channel, layout):
    film, rgb = yard.restated_render(channel, "sky", _ld, "counter")[2:4]

    def run():
        out = yard.renderer(channel, _ld).render(yard.scene["sky"])
        return out, yard.scene["sky"]._device().last_render_info()
    out, info = _with_option("DARTRAY_STATE_LAYOUT", layout, run)
    assert info["state_layout"] == layout and _same(out.film, film) and _same(out.rgb, rgb)


@pytest.mark.parametrize("channel", CHANNELS)
def test_a_gaussian_film_at_the_splats_tolerance(yard, channel):
    filt = core.GaussianFilter(2.0, 2.0, 2.0)
    Ls, hit, film, rgb, pixels, vec = yard.restated_render(channel, "sky", _ld, "counter-gauss", filt)
    out = yard.renderer(channel, _ld, yard.camera(filt)).render(yard.scene["sky"])
    err = np.abs(out.film - film)
    print("gaussian %s film: max |device - restatement| = %.3g, max relative = %.3g" % (channel, err.max(), (err / np.maximum(np.abs(film), 1e-30)).max()))
    assert np.allclose(out.film, film, rtol=2e-5, atol=2e-6) and np.allclose(out.rgb, rgb, rtol=2e-5, atol=2e-6)
    assert not _same(film, yard.restated_render(channel, "sky", _ld, "counter")[2])


# ---- 4. the black-scene identity ----
BLACK = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def black_box(gpu):
    """Cornell walls and a block, every material Kd = 0, one area light in view and no infinite light: nothing reflects, so Li of the camera
    ray is the emitted term alone."""
    quad = lambda P, light=None: mc.mesh(P, core.MatteMaterial(BLACK), light=light)
    s = 10.0
    prims = [quad([(-s, -s, -s), (s, -s, -s), (s, -s, s), (-s, -s, s)]), quad([(-s, -s, s), (s, -s, s), (s, s, s), (-s, s, s)]),
             quad([(-s, -s, -s), (-s, -s, s), (-s, s, s), (-s, s, -s)]), quad([(s, -s, -s), (s, s, -s), (s, s, s), (s, -s, s)]),
             quad([(-4.0, -2.0, 2.0), (4.0, -2.0, 2.0), (4.0, 5.0, 6.0), (-4.0, 5.0, 6.0)][::-1], core.DiffuseAreaLight((36.0, 30.0, 24.0), 1))]
    return scenes.make_scene(prims)


@pytest.mark.parametrize("name", ["path", "direct_all", "direct_one", "whitted"])
def test_in_a_black_scene_the_emission_image_is_the_beauty_image(black_box, name):
    integ = {"path": lambda: core.PathIntegrator(3), "direct_all": lambda: core.DirectLightingIntegrator(0, 3),
             "direct_one": lambda: core.DirectLightingIntegrator(1, 3), "whitted": lambda: core.WhittedIntegrator(3)}[name]()
    cam = scenes.cornell_camera(16, 16)
    beauty = core.SamplerRenderer(_ld(cam), cam, integ, core.EmissionIntegrator()).render(black_box)
    emission = core.SamplerRenderer(_ld(cam), cam, core.MaterialIntegrator("emission"), core.EmissionIntegrator()).render(black_box)
    lit = (emission.rgb > 0).any(axis=2)
    assert 8 < lit.sum() < 236 and np.isfinite(beauty.rgb).all()                # the emitter and black both in view
    assert np.array_equal(emission.rgb, beauty.rgb) and np.array_equal(emission.film, beauty.film)
    albedo = core.SamplerRenderer(_ld(cam), cam, core.MaterialIntegrator("albedo"), core.EmissionIntegrator()).render(black_box)
    assert not albedo.rgb.any()


# ---- 5. the refusals, by code and text; what ran ----
def test_refusals_by_name_leave_the_scene_usable(yard):
    lib = _abi.lib()
    film = np.zeros((16, 16, 4), np.float32)
    scene = yard.scene["sky"]

    def refused(code, needle, mutate):
        d, keep = yard.renderer("albedo", _ld).describe()
        mutate(d)
        rc = lib.dr_render(scene._device().handle, C.byref(d), film.ctypes.data, None)
        assert rc == code, rc
        assert needle in lib.dr_last_error().decode(), lib.dr_last_error()

    def adaptive(d):
        d.sampler_mode, d.spp, d.strat_xsamples = _abi.DR_SAMPLER_ADAPTIVE, 8, 2
    refused(-4, "material integrator: the adaptive sampler is not supported", adaptive)
    for ch in (2, -1, 1 << 20):
        refused(-1, "material integrator: unknown channel", lambda d: setattr(d, "material_channel", ch))
    assert not film.any()
    d, keep = yard.renderer("albedo", _ld).describe()
    _abi.check(lib.dr_render(scene._device().handle, C.byref(d), film.ctypes.data, None))
    assert _same(film, yard.restated_render("albedo", "sky", _ld, "counter")[2])


def test_last_render_info_names_the_integrator_and_its_kernel(yard):
    scene = yard.scene["sky"]
    for channel, const in (("albedo", _abi.DR_MATERIAL_CHANNEL_ALBEDO), ("emission", _abi.DR_MATERIAL_CHANNEL_EMISSION)):
        r = yard.renderer(channel, _ld)
        r.render(scene)
        info = scene._device().last_render_info()
        assert info["integrator"] == "material" and info["shade_kernels"] == ["k_shade_material"] and info["material_channel"] == const
        assert info["feature_channel"] is None
        st = r.last_stats
        hits = int(yard.restated_render(channel, "sky", _ld, "counter")[1].sum())
        assert st["camera_samples"] == 17 * 17 * 2 == st["shade_items"] and st["shade_vertices"] == hits
        assert st["closest_launches"] == 1 and st["any_launches"] == 0 and st["any_rays"] == 0  # the camera rays and nothing else
    core.SamplerRenderer(_ld(yard.camera()), yard.camera(), core.FeatureIntegrator("depth"), core.EmissionIntegrator()).render(scene)
    assert scene._device().last_render_info()["material_channel"] is None
