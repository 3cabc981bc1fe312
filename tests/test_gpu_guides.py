"""Guide images in the beauty render's own pass on the GPU (dr_render_guides*, k_guides): every guide of
SamplerRenderer.render_with_guides against the separate FeatureIntegrator render it replaces (_image._rerender), and the beauty image against
render().  24 x 20 films (a 25 x 21 sampler window: neither side a multiple of a 64-slot tile or of the other) over one small scene: a mesh
with per-vertex N and uvs, meshes without, a sphere, a disk, a mirror quad, and pixels that hit nothing -- and the same scene without its two
quadrics, which alone takes the default routes of a triangle scene (k_trace_pk for the camera rays, lazy sample generation).  Under the box filter of width 0.5
every sample lands in its own pixel, which the film adds in one serial chain (k_film), so films and images are compared
byte for byte.  A feature render is computed once per (sampler, setting, channel) and shared.  Nothing is started after a failed call:
every call's return code raises."""
import numpy as np
import pytest

from dartray_amd import _abi, core, denoise, pbrt
from dartray_amd._image import _rerender

pytestmark = pytest.mark.gpu

SEED = 5489
CHANNELS = ("ng", "ns", "depth", "uv", "id")
GREY = (0.5, 0.5, 0.5)
T = pbrt.Transform
W, H = 24, 20


def _mesh(P, idx=((0, 1, 2), (0, 2, 3)), material=None, **kw):
    return core.GeometricPrimitive(core.TriangleMesh(np.array(idx, np.uint32), np.array(P, np.float32), **kw), material or core.MatteMaterial(GREY), None)


def _prims(quadrics=True):
    n = np.array([(0.3, 0.9, -0.1), (-0.2, 0.8, -0.4), (-0.3, 0.7, -0.6), (0.4, 0.9, -0.2)], np.float32)
    prims = [_mesh([(-4.0, 0.0, -2.0), (-4.0, 0.0, 5.0), (4.0, 0.0, 5.0), (4.0, 0.0, -2.0)]),                      # the floor: no N, no uvs
             _mesh([(-3.0, 0.5, 2.5), (-0.5, 0.5, 2.5), (-0.5, 2.5, 3.5), (-3.0, 2.5, 3.5)], n=n,                  # per-vertex N and uvs
                   uvs=np.array([(0.0, 0.0), (2.0, 0.0), (2.0, 1.5), (0.0, 1.5)], np.float32)),
             _mesh([(0.5, 0.2, 1.0), (2.5, 0.2, 1.0), (2.5, 1.8, 2.0), (0.5, 1.8, 2.0)], material=core.MirrorMaterial((0.9, 0.9, 0.9))),
             _mesh([(-1.0, 0.1, 0.2), (0.6, 0.1, 0.0), (-0.2, 1.2, 0.6)], idx=((0, 1, 2),), reverseOrientation=True)]
    if not quadrics:
        return prims
    at = T.Translate(1.6, 2.6, 3.0)
    prims.append(core.GeometricPrimitive(core.Sphere(at.m, at.mInv, False, 0.9), core.MatteMaterial(GREY), None))
    up = T.Translate(-2.0, 3.2, 3.0) * T.Rotate(60.0, 1.0, 0.0, 0.0)
    prims.append(core.GeometricPrimitive(core.Disk(up.m, up.mInv, True, 0.0, 0.8, 0.2), core.MatteMaterial(GREY), None))
    return prims


INTEGRATORS = {"path": lambda: core.PathIntegrator(3), "direct_all": lambda: core.DirectLightingIntegrator(0, 3),
               "direct_one": lambda: core.DirectLightingIntegrator(1, 3), "whitted": lambda: core.WhittedIntegrator(3),
               "ao": lambda: core.AmbientOcclusionIntegrator(4)}


def _ld(spp):
    return lambda cam: core.LowDiscrepancySampler(cam, spp, SEED)


def _camera(filt=None, w=W, h=H, eye=(0.0, 3.0, -6.0)):
    return core.PerspectiveCamera.lookAt(eye, (0.0, 1.2, 2.0), (0.0, 1.0, 0.0), 50.0, core.ImageFilm(w, h, filt or core.BoxFilter(0.5, 0.5)))


class Yard:
    def __init__(self, quadrics=True):
        self.accel = core.BVHAccel(_prims(quadrics))
        self.scene = core.Scene(self.accel, [core.PointLight(T.Translate(0.0, 6.0, -3.0).m, (30.0, 30.0, 30.0))])
        self.features = {}

    def renderer(self, integrator, mk_sampler, cam=None, **kw):
        cam = cam or _camera()
        surface = INTEGRATORS[integrator]() if isinstance(integrator, str) else integrator
        return core.SamplerRenderer(mk_sampler(cam), cam, surface, core.EmissionIntegrator(), **kw)

    def feature(self, key, renderer, channel):
        """The separate FeatureIntegrator render of `channel` beside `renderer`, as _image._guides makes it; computed once per key."""
        k = (key, channel)
        if k not in self.features:
            self.features[k] = _rerender(renderer, self.scene, core.FeatureIntegrator(channel))
        return self.features[k]


@pytest.fixture(scope="module")
def yard(gpu):
    return Yard()


@pytest.fixture(scope="module")
def tris(gpu):
    """The same meshes, the mirror and the misses without the sphere and the disk: a scene with a quadric never takes the wave-coherent camera
    traversal (k_trace_pk) nor lazy sample generation, the routes a triangle-only scene takes by default."""
    return Yard(quadrics=False)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _option(name, value):
    _abi.check(_abi.lib().dr_set_option(name.encode(), None if value is None else str(value).encode()))


def _check(yard, key, renderer, channels=CHANNELS, same=_same):
    """Tests 1 and 2 of the issue for one renderer: every guide equals the feature render, the beauty image equals render()."""
    got = renderer.render_with_guides(yard.scene, channels)
    info = yard.scene._device().last_render_info()
    assert tuple(got.guides) == tuple(channels) == tuple(got.guide_films)
    for ch in channels:
        want = yard.feature(key, renderer, ch)
        assert same(got.guide_films[ch], want.film), (key, ch, "film")
        assert same(got.guides[ch], want.rgb), (key, ch, "rgb")
    plain = renderer.render(yard.scene)
    assert same(got.film, plain.film) and same(got.rgb, plain.rgb), (key, "beauty")
    assert np.isfinite(got.film).all() and got.film[..., 3].sum() > 0
    return got, info


# ---- 1 + 2. every accepted integrator, both film paths ----
@pytest.mark.parametrize("spp", [1, 4, 64])
@pytest.mark.parametrize("integrator", sorted(INTEGRATORS))
def test_guides_equal_the_feature_renders_and_the_beauty_image_is_untouched(yard, integrator, spp):
    got, info = _check(yard, ("ld", spp), yard.renderer(integrator, _ld(spp)))
    assert info["batches"] == 1
    depth, ids = got.guides["depth"][..., 0], got.guide_films["id"]
    assert (depth > 0).sum() > 100 and (depth == 0).sum() > 20                       # hits and misses both
    assert not _same(got.guides["ng"], got.guides["ns"])                              # the mesh with N
    assert got.guides["uv"][..., 0].max() > 1.0                                       # ... and its own uvs
    assert ids[..., 2].max() > 0 and got.rgb.max() > 0


def test_the_guide_of_a_mirror_is_the_mirror(yard):
    """DirectLighting over mirror / glass runs rounds of the stage loop (k_shade_spec); the guide is the first hit, as under the feature
    integrator: the id image names the mirror quad's two triangles where the camera sees it."""
    r = yard.renderer("direct_all", _ld(1))
    got = r.render_with_guides(yard.scene, ("id",))
    mats = np.rint(got.guides["id"][..., 1]).astype(int)
    mirror = next(i for i, m in enumerate(yard.accel.materials) if isinstance(m, core.MirrorMaterial)) + 1
    assert (mats == mirror).sum() > 4
    assert _same(got.guide_films["id"], yard.feature(("ld", 1), r, "id").film)


# ---- 3. batches ----
@pytest.mark.parametrize("integrator", ["path", "direct_all", "ao"])
def test_a_frame_of_several_batches(yard, integrator):
    """DARTRAY_BATCH_BITS=8 as the issue states it; the library clamps the switch to 16 (include/dartray_hip.h: 16..28), so the 4-spp frame --
    525 pixels, 2100 slots -- stays one batch.  It is rendered under the switch all the same, and the frame that does span several batches at
    this film size is rendered too: 256 spp, 134 400 slots, three batches of 2^16 at most."""
    try:
        _option("BATCH_BITS", 8)
        _check(yard, ("ld", 4), yard.renderer(integrator, _ld(4)))
        got, info = _check(yard, ("ld", 256), yard.renderer(integrator, _ld(256)))
        assert info["batches"] > 1, info
    finally:
        _option("BATCH_BITS", None)


# ---- 4. layouts and the camera route ----
@pytest.mark.parametrize("name,value", [("STATE_LAYOUT", 64), ("STATE_LAYOUT", 4), ("COHERENT_CAMERA", 0)])
def test_state_layouts_and_the_per_lane_camera_traversal(yard, name, value):
    r = yard.renderer("path", _ld(4))
    for ch in CHANNELS:
        yard.feature(("ld", 4), r, ch)          # (the references under the defaults)
    try:
        _option(name, value)
        got, info = _check(yard, ("ld", 4), r)
        if name == "STATE_LAYOUT":
            assert info["state_layout"] == value
        else:
            assert info["coherent_camera"] == 0
    finally:
        _option(name, None)


# ---- 4b. the default routes of a triangle-only scene: k_trace_pk in front of the seam, lazy sample generation behind it ----
@pytest.mark.parametrize("layout", [None, 64, 4])
@pytest.mark.parametrize("spp", [4, 64, 256])
def test_behind_the_coherent_camera_traversal_and_under_lazy_generation(tris, spp, layout):
    """Path over triangles only: the camera rays go through k_trace_pk (last_render_info says so), and from 64 spp on the bounce blocks are
    generated lazily -- the state carries k_trace_pk's marks when k_guides runs, and genBounce(0) follows right behind it.  256 spp under
    DARTRAY_BATCH_BITS=16 is three such batches.  In the layout the render picks and in both forced ones."""
    r = tris.renderer("path", _ld(spp))
    for ch in CHANNELS:
        tris.feature(("ld", spp), r, ch)          # (the references under the defaults)
    try:
        if layout is not None:
            _option("STATE_LAYOUT", layout)
        if spp == 256:
            _option("BATCH_BITS", 16)
        got, info = _check(tris, ("ld", spp), r)
    finally:
        _option("STATE_LAYOUT", None)
        _option("BATCH_BITS", None)
    assert info["coherent_camera"] == 1, info
    assert info["lazy_gen"] == (1 if spp >= 64 else 0), info
    assert layout is None or info["state_layout"] == layout
    assert info["batches"] == (3 if spp == 256 else 1), info
    depth = got.guides["depth"][..., 0]
    assert (depth > 0).sum() > 100 and (depth == 0).sum() > 20 and not _same(got.guides["ng"], got.guides["ns"])


@pytest.mark.parametrize("layout", [64, 4])
def test_the_switch_takes_a_triangle_scene_off_the_coherent_route(tris, layout):
    """DARTRAY_COHERENT_CAMERA=0 on the scene where it changes the route: the per-lane kernels trace the camera rays, nothing is generated
    lazily, and guides and beauty image are the bytes of the default route (the references were rendered under the defaults)."""
    r = tris.renderer("path", _ld(64))
    default = r.render_with_guides(tris.scene, CHANNELS)
    assert tris.scene._device().last_render_info()["coherent_camera"] == 1
    try:
        _option("COHERENT_CAMERA", 0)
        _option("STATE_LAYOUT", layout)
        got, info = _check(tris, ("ld", 64), r)
    finally:
        _option("COHERENT_CAMERA", None)
        _option("STATE_LAYOUT", None)
    assert info["coherent_camera"] == 0 and info["lazy_gen"] == 0 and info["state_layout"] == layout, info
    assert _same(got.film, default.film) and all(_same(got.guide_films[ch], default.guide_films[ch]) for ch in CHANNELS)


@pytest.mark.parametrize("integrator", ["direct_one", "ao"])
def test_other_integrators_behind_the_coherent_camera_traversal(tris, integrator):
    """No mirror recursion under these two (DirectLighting "one" over the mirror runs k_shade_spec's rounds and so the per-lane kernels; ambient
    occlusion does not): whichever route the planner picks, the guides are the feature renders'."""
    got, info = _check(tris, ("ld", 4), tris.renderer(integrator, _ld(4)))
    assert info["coherent_camera"] == (1 if integrator == "ao" else 0), info


# ---- 5. samplers ----
def _splat_close(a, b):
    """A film that is summed by f32 atomics in no fixed order, as tests/test_gpu_filters.py compares one (rtol 2e-5, atol 2e-6)."""
    return np.allclose(a, b, rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("name", ["stratified", "random", "replay"])
def test_pixel_bound_samplers(yard, name):
    if name == "replay":
        # the LD sampler's own vectors for a PathIntegrator(2) -- no RNG tail below three bounces -- replayed through host buffers
        src = yard.renderer(core.PathIntegrator(2), _ld(4))
        pixels = src.pixels()
        vec = src.generate_samples(yard.scene, pixels)
        r = yard.renderer(core.PathIntegrator(2), lambda cam: core.HostBufferSampler(cam, 4, pixels, vec))
    else:
        mk = {"stratified": lambda cam: core.StratifiedSampler(cam, 2, 2, True, SEED), "random": lambda cam: core.RandomSampler(cam, 4, SEED)}[name]
        r = yard.renderer("path", mk)
    _check(yard, (name, 4), r, ("ns", "depth"))


def test_the_halton_sampler(yard):
    """5 pixelsamples: no power of two.  The Halton sampler's slots are single samples, so k_film adds every one of them to its pixel by an f32
    atomic in no fixed order -- two renders of one frame already differ -- and the comparison is the splats' (tests/test_gpu_filters.py;
    tests/test_gpu_feature.py::test_halton_sampler_renders compares its film the same way); the weights are counts and equal exactly."""
    r = yard.renderer("path", lambda cam: core.HaltonSampler(cam, 5, SEED))
    got, _ = _check(yard, ("halton", 5), r, ("ns", "depth"), same=_splat_close)
    for ch in ("ns", "depth"):
        assert np.array_equal(got.guide_films[ch][..., 3], yard.feature(("halton", 5), r, ch).film[..., 3])
        assert np.array_equal(got.guide_films[ch][..., 3], got.film[..., 3]) and got.film[..., 3].sum() > 500


# ---- 6. windows ----
@pytest.mark.parametrize("task", [0, 1])
def test_each_task_of_two_has_its_own_guides(yard, task):
    r = yard.renderer("path", _ld(4), taskNum=task, taskCount=2)
    got, _ = _check(yard, ("ld-task", task), r, ("ns", "depth"))
    assert 0 < (got.film[..., 3] > 0).sum() < W * H


# ---- 7. a render without guides is unchanged ----
def test_a_render_without_guides_allocates_and_launches_nothing_new(gpu, capfd):
    def fresh():
        return core.Scene(core.BVHAccel(_prims()), [core.PointLight(T.Translate(0.0, 6.0, -3.0).m, (30.0, 30.0, 30.0))])
    cam = _camera()
    r = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 4, SEED), cam, core.PathIntegrator(3), core.EmissionIntegrator())
    never, seen = fresh(), fresh()
    r.render(never)
    base = never._device().workspace_bytes()
    r.render_with_guides(seen, ("ns", "depth"))
    with_guides = seen._device().workspace_bytes()
    r.render(seen)
    assert with_guides == base + 2 * 3 * 4 * 2112                     # two planes of three floats for 2100 slots in whole tiles
    third = fresh()
    r.render(third)
    assert third._device().workspace_bytes() == base and base > 0
    try:
        _option("STAGE_COUNTS", 1)
        capfd.readouterr()
        r.render(never)
        plain = capfd.readouterr().err
        r.render_with_guides(seen, ("ns", "depth"))
        guided = capfd.readouterr().err
    finally:
        _option("STAGE_COUNTS", "")
    assert "stage_counts batch" in plain and "guides" not in plain
    assert "stage_times batch 1 guides: 2 channels" in guided
    strip = lambda text: [line for line in text.splitlines() if "guides" not in line and line.startswith("stage_counts")]
    assert strip(plain) == strip(guided)


# ---- 8. the pipeline ----
def _pipeline_renderer(seed, w=W, h=H, eye=(0.0, 3.0, -6.0)):
    cam = _camera(w=w, h=h, eye=eye)
    return core.SamplerRenderer(core.LowDiscrepancySampler(cam, 4, seed), cam, core.PathIntegrator(3), core.EmissionIntegrator())


def _same_parts(a, b, names):
    return all(_same(getattr(a, n), getattr(b, n)) for n in names)


def test_the_pipeline_functions_return_the_same_bytes_in_one_pass(yard):
    r = _pipeline_renderer(SEED)
    parts = ("rgb", "noisy", "normal", "depth")
    assert _same_parts(denoise.render_denoised(r, yard.scene, one_pass=True, iterations=2), denoise.render_denoised(r, yard.scene, iterations=2), parts)
    assert _same_parts(denoise.render_denoised(r, yard.scene, normal_channel="ng", one_pass=True, iterations=2),
                       denoise.render_denoised(r, yard.scene, normal_channel="ng", one_pass=False, iterations=2), parts)
    assert _same_parts(denoise.render_denoised_pair(r, yard.scene, one_pass=True, iterations=2), denoise.render_denoised_pair(r, yard.scene, iterations=2),
                       parts + ("a", "b", "variance"))
    assert _same_parts(denoise.render_firefly(r, yard.scene, one_pass=True), denoise.render_firefly(r, yard.scene), parts + ("removed",))
    low = _pipeline_renderer(SEED, W // 2, H // 2)
    assert _same_parts(denoise.render_upsampled(low, r, yard.scene, one_pass=True), denoise.render_upsampled(low, r, yard.scene),
                       ("rgb", "low", "normal_lo", "depth_lo", "normal", "depth", "upsampled"))


def test_a_sequence_returns_the_same_bytes_in_one_pass(yard):
    """A static pair and one moved pose.  The second frame's sampler has a seed of its own: its guides are sampled with the first frame's and
    stay feature renders; the first and the third take theirs from the beauty render."""
    renderers = [_pipeline_renderer(SEED), _pipeline_renderer(77), _pipeline_renderer(SEED, eye=(0.4, 3.0, -6.0))]
    one, three = denoise.render_sequence(renderers, yard.scene, one_pass=True), denoise.render_sequence(renderers, yard.scene)
    assert len(one) == 3
    for a, b in zip(one, three):
        assert _same_parts(a, b, ("rgb", "noisy", "normal", "depth", "accumulated", "m2", "len"))
    assert (one[1].len == 2).any() and not _same(one[0].normal, one[2].normal)


# ---- 9. a wide filter ----
def test_a_gaussian_film_at_the_splats_tolerance(yard):
    """A filter whose support crosses pixels: every sample also goes to foreign pixels by f32 atomics in no fixed order, so two renders of one
    frame differ in summation order.  Compared as tests/test_gpu_filters.py compares a wide-filter film: np.allclose(rtol=2e-5, atol=2e-6)."""
    cam = _camera(core.GaussianFilter(2.0, 2.0, 2.0))
    r = yard.renderer("path", _ld(4), cam)
    got, _ = _check(yard, ("ld-gauss", 4), r, ("ns", "depth"), same=_splat_close)
    assert not _same(got.guide_films["depth"], yard.feature(("ld", 4), yard.renderer("path", _ld(4)), "depth").film)
