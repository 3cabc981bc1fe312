"""What the wrappers of the image-space stages share (denoise.py, display.py; DESIGN.md 2.15, "what an image stage is made of"): the entry
point of a stage on the device or on the host, the conversion and shape check of its images, the guide images a render_* function renders
beside the beauty image, and the refusals of the functions that need the whole film in one piece."""
import numpy as np

from . import _abi
from .core.renderer import FeatureIntegrator, SamplerRenderer
from .core.samplers import AdaptiveSampler


def _entry(name, device):
    """The library's `name` (device=True: on the GPU, initialised if nothing has) or `name`_host, which needs none."""
    lib = _abi.lib()
    if device:
        _abi.init(_abi._initialised if _abi._initialised is not None else 0)
    return getattr(lib, name if device else name + "_host")


def _images(who, what, rgb3s, plane=None):
    """rgb3s, then plane where given, as contiguous f32 arrays: the first [h, w, 3], the others of its shape, the plane [h, w].  `what`
    is the refusal's wording."""
    out = [np.ascontiguousarray(a, dtype=np.float32) for a in list(rgb3s) + ([] if plane is None else [plane])]
    first, n = out[0], len(rgb3s)
    if first.ndim != 3 or first.shape[2] != 3 or any(a.shape != first.shape for a in out[1:n]) or any(a.shape != first.shape[:2] for a in out[n:]):
        raise ValueError("%s: %s (got %s)" % (who, what, ", ".join("%r" % (a.shape,) for a in out)))
    return out


def _check_channel(who, normal_channel):
    if normal_channel not in ("ns", "ng"):
        raise ValueError("%s: normal_channel must be ns or ng (got %r)" % (who, normal_channel))


def _rerender(renderer, scene, surface, sampler=None):
    """`renderer`'s camera, volume integrator and work split around another surface integrator (and sampler), rendered."""
    r = renderer
    return SamplerRenderer(r.sampler if sampler is None else sampler, r.camera, surface, r.volumeIntegrator, taskNum=r.taskNum,
                           taskCount=r.taskCount, tileRank=r.tileRank, tileCount=r.tileCount, tileSize=r.tileSize).render(scene)


def _guides(renderer, scene, normal_channel, sampler=None):
    """(normal [h, w, 3], depth [h, w]): the two FeatureIntegrator images every stage is guided by."""
    normal = _rerender(renderer, scene, FeatureIntegrator(normal_channel), sampler).rgb
    return normal, np.ascontiguousarray(_rerender(renderer, scene, FeatureIntegrator("depth"), sampler).rgb[..., 0])


def _check_one_pass(who, one_pass, renderer=None, scene=None, normal_channel="ns"):
    """The `one_pass` keyword of a render_* function: a bool, and -- True with a renderer -- one that dr_render_guides_check accepts for
    `renderer` (its refusal raises ValueError naming the integrator or the sampler, before anything is rendered)."""
    if one_pass is not True and one_pass is not False:
        raise ValueError("%s: one_pass must be False or True, got %r" % (who, one_pass))
    if one_pass and renderer is not None:
        try:
            renderer.guides_desc(scene, (normal_channel, "depth"))
        except ValueError as e:
            raise ValueError("%s: one_pass=True: %s" % (who, e)) from e


def _render_with_guides(renderer, scene, normal_channel):
    """(beauty OutputImage, normal [h, w, 3], depth [h, w]) from ONE render of `renderer` (SamplerRenderer.render_with_guides):
    the beauty image render() returns and the two images _guides renders separately."""
    beauty = renderer.render_with_guides(scene, (normal_channel, "depth"))
    return beauty, beauty.guides[normal_channel], np.ascontiguousarray(beauty.guides["depth"][..., 0])


def _beauty_and_guides(renderer, scene, normal_channel, one_pass):
    """(beauty, normal, depth): three renders, or with one_pass one."""
    if one_pass:
        return _render_with_guides(renderer, scene, normal_channel)
    beauty = renderer.render(scene)
    normal, depth = _guides(renderer, scene, normal_channel)
    return beauty, normal, depth


def _whole_film_refusals(who, name, r, what, each=True):
    """What a function that cannot work on a part of the film asks of renderer `r`, called `name` in the refusal.  `what` is the stage's
    noun; each=False names tileCount and taskCount in one refusal."""
    if isinstance(r.sampler, AdaptiveSampler):
        raise ValueError("%s: the adaptive sampler is not supported (%s; the feature integrator refuses it)" % (who, name))
    if not each and (r.tileCount > 1 or r.taskCount > 1):
        raise ValueError("%s: tileCount > 1 and taskCount > 1 are not supported (%s has %d and %d): sharded %s is out of scope"
                         % (who, name, r.tileCount, r.taskCount, what))
    for count in ("tileCount", "taskCount"):
        if getattr(r, count) > 1:
            raise ValueError("%s: %s > 1 is not supported (%s has %s %d): sharded %s is out of scope" % (who, count, name, count, getattr(r, count), what))
    crop = tuple(r.camera.film.cropWindow)
    if crop != (0.0, 1.0, 0.0, 1.0):
        raise ValueError("%s: a crop window other than the whole film is not supported (%s has %r)" % (who, name, crop))
