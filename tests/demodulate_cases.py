"""The inputs the demodulation tests share (tests/test_demodulate.py on the host, tests/test_gpu_demodulate.py on the device): seeded images
at the three sizes, with every special pixel the rule names placed at a pixel of its own."""
import numpy as np

F = np.float32
EPS = 1.0e-3
SIZES = [(1, 1), (3, 5), (67, 9)]                                  # (w, h); 67 x 9: no tile and no wave divides it
ABSENT = {"both": (True, True), "no_emission": (False, True), "no_albedo": (True, False), "neither": (False, False)}

NAN, INF = F(np.nan), F(np.inf)


def _zero_albedo(rgb, e, a, p):
    a[p] = 0.0
    e[p] = 0.0                                                     # a lit pixel over a black surface: divided by eps alone


def _one_ulp_below(rgb, e, a, p):
    e[p] = (0.5, 1.0, 36.0)
    rgb[p] = np.nextafter(e[p], F(0), dtype=F)                     # rgb < e by one ulp in every channel: clamped to 0


def _pure_emitter(rgb, e, a, p):
    e[p] = (36.0, 36.0, 36.0)
    rgb[p] = e[p]


def _set(which, value, channel):
    def f(rgb, e, a, p):
        (rgb, e, a)[which][p][channel] = value
    return f


SPECIALS = [_zero_albedo, _one_ulp_below, _pure_emitter,
            _set(0, NAN, 0), _set(0, INF, 1), _set(1, NAN, 2), _set(1, -INF, 0), _set(2, NAN, 1), _set(2, INF, 2)]


def images(w, h):
    """A list of (rgb, emission, albedo) [h, w, 3] f32 triples that between them hold every special pixel: one triple where the image has
    room for all nine, one per special at 1 x 1."""
    n = w * h
    per = min(n, len(SPECIALS))
    out = []
    for first in range(0, len(SPECIALS), per):
        rng = np.random.default_rng(1000 * w + h + first)
        rgb = (rng.random((n, 3)) * 4.0).astype(F)
        e = np.where(rng.random((n, 1)) < 0.3, rng.random((n, 3)) * 2.0, 0.0).astype(F)
        a = rng.random((n, 3)).astype(F)
        for k, special in enumerate(SPECIALS[first:first + per]):
            special(rgb, e, a, (k * 7 + 3) % n if n >= len(SPECIALS) else k)
        out.append(tuple(x.reshape(h, w, 3) for x in (rgb, e, a)))
    return out


def exact_images(w, h):
    """(rgb, emission, albedo, eps) for which remodulate(demodulate(x)) == x bit for bit: rgb and e are multiples of 2^-10 below 8 with
    rgb >= e, so the subtraction and the addition are exact, and a + eps is a power of two (eps = 0.25), so the division and the product are."""
    rng = np.random.default_rng(7 * w + h)
    e = (rng.integers(0, 2048, (h, w, 3)) / 1024.0).astype(F)
    rgb = e + (rng.integers(0, 4096, (h, w, 3)) / 1024.0).astype(F)
    a = rng.choice(np.array([0.25, 0.75, 1.75, 3.75], F), (h, w, 3))
    return rgb.astype(F), e, a.astype(F), 0.25


def same(x, y):
    return np.array_equal(np.ascontiguousarray(x, F).view(np.uint32), np.ascontiguousarray(y, F).view(np.uint32))


LEMIT = (36.0, 36.0, 36.0)


def emitter_box_prims():
    """A Cornell-like box of matte walls (Kd 0.4; the side walls tinted) open towards the camera of scenes.cornell_camera, with a 10 x 10
    emitter of Lemit 36 set into the back wall and facing the camera.  The emitter's own surface is black, so a pixel wholly inside it
    holds Lemit and nothing else in the unfiltered render; at 32 x 32 it covers the ten pixels 11 .. 20 in both axes entirely."""
    from dartray_amd import core
    s, h, kd = 10.0, 5.0, 0.4

    def quad(P, colour, light=None):
        mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array(P, np.float32))
        return core.GeometricPrimitive(mesh, core.MatteMaterial(colour), light)
    W = (kd, kd, kd)
    return [quad([(-s, -s, -s), (s, -s, -s), (s, -s, s), (-s, -s, s)], W), quad([(-s, s, -s), (-s, s, s), (s, s, s), (s, s, -s)], W),
            quad([(-s, -s, s), (s, -s, s), (s, s, s), (-s, s, s)], W), quad([(-s, -s, -s), (-s, -s, s), (-s, s, s), (-s, s, -s)], (kd, 0.1, 0.1)),
            quad([(s, -s, -s), (s, s, -s), (s, s, s), (s, -s, s)], (0.1, kd, 0.1)),
            quad([(-h, h, 9.9), (h, h, 9.9), (h, -h, 9.9), (-h, -h, 9.9)], (0.0, 0.0, 0.0), core.DiffuseAreaLight(LEMIT, 1))]


INSIDE = (slice(11, 21), slice(11, 21))                            # the pixels wholly inside the emitter at 32 x 32
EMITTER_RTOL, EMITTER_ATOL = 2e-5, 2e-6                            # the splats' tolerance (tests/test_gpu_material.py)
