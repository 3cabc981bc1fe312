"""Writes sampler_modes.npz: what the device does in every sampler mode (host buffer, low-discrepancy, stratified, adaptive, Halton) on
C1 at 16 x 12 with the box filter -- film, image, dr_scene_last_render_info, the sample counts and the sampler's own dump -- plus two
two-batch renders at 40 x 32 and the (return code, message) pair of every refused descriptor.  A frozen picture of the commit it was run
at: tests/test_gpu_sampler_modes.py collects the same entries again and compares.  Needs a GPU; run by hand, once:

    python tests/golden/make_sampler_mode_goldens.py

Every entry is collected twice and the script aborts if the two differ in a bit.  Halton films are the exception (samples are not grouped
by pixel, so the order of a pixel's atomic additions is free, tests/test_gpu_halton.py): their colour channels are stored with the bound
(2 n + 4) 2^-24 S of tests/film_reference.py, from the oracle's radiances of the restated samples."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from dartray_amd import _abi, core, scenes  # noqa: E402

OUT = os.path.join(HERE, "sampler_modes.npz")
PIXELS = np.array([(0, 0), (1, 0), (16, 12), (7, 11), (15, 3)], np.int32)  # the dumps' pixels: corners of the 17 x 13 sampler window and inside


def c1(integ, nsamples=1, xres=16, yres=12, spp=4):
    """C1 under PathIntegrator(5) ("path") or DirectLighting "all" / "one", the emitter at `nsamples` samples."""
    prims, mk = scenes.config("C1", xres=xres, yres=yres, spp=spp)
    next(gp for gp in prims if gp.areaLight is not None).areaLight.nSamples = nsamples
    r = mk()
    r.surfaceIntegrator = core.PathIntegrator(5) if integ == "path" else core.DirectLightingIntegrator(int(integ == "one"), 5)
    return prims, r


def samplers(r):
    return {"ld": lambda: core.LowDiscrepancySampler(r.camera, 4, 5489), "strat": lambda: core.StratifiedSampler(r.camera, 2, 2, True, 5489),
            "strat_nojitter": lambda: core.StratifiedSampler(r.camera, 2, 2, False, 5489),
            "adaptive": lambda: core.AdaptiveSampler(r.camera, 2, 8, "contrast", 5489), "halton": lambda: core.HaltonSampler(r.camera, 3, 5489)}


def info_words(scene):
    arr = (C.c_int32 * 8)()
    _abi.check(_abi.lib().dr_scene_last_render_info(scene._device().handle, C.byref(arr)))
    return np.array(arr[:], np.int32)


def rendered(r, scene, rgb=True):
    out = r.render(scene)
    got = {"film": out.film, "info": info_words(scene),
           "counts": np.array([r.last_stats[k] for k in ("camera_samples", "film_samples", "batches")], np.int64)}
    if rgb:
        got["rgb"] = out.rgb
    return got


# sampler -> its integrators, light nsamples (entries 1 to 4 of the issue's table)
MODES = [("ld", "path", 1), ("ld", "all", 1), ("ld", "one", 1), ("strat", "path", 1), ("strat", "all", 4), ("strat_nojitter", "path", 1),
         ("strat_nojitter", "all", 4), ("adaptive", "path", 1), ("adaptive", "all", 1), ("halton", "path", 1), ("halton", "all", 4)]


def mode_entry(sampler, integ, nsamples):
    prims, r = c1(integ, nsamples)
    r.sampler = samplers(r)[sampler]()
    scene = scenes.make_scene(prims)
    got = rendered(r, scene, rgb=sampler != "halton")
    if sampler == "adaptive":
        xy = r.supersampled_pixels(scene)
        got["supersampled"] = xy[np.lexsort((xy[:, 0], xy[:, 1]))]
    if sampler == "halton":
        got["dump_k"], got["dump_xy"], got["dump"] = r.generate_halton_samples(scene)
    else:
        got["dump"] = r.generate_samples(scene, PIXELS)
    return got


def serial_recording(ob):
    """The reference's serial stream of the ld / path case, recorded by the oracle in tile order -> (prims, renderer with the packed-tail
    HostBufferSampler of the recording)."""
    prims, r = c1("path")
    r.sampler.pixelSampler = core.TilePixelSampler()
    rec = ob.OracleScene(prims).render(ob.render_desc(r, sampler_mode=0), record=17 * 13 * 4, max_tail=40)
    r.sampler = core.HostBufferSampler(r.camera, 4, rec["pixel_xy"][::4], rec["sample_vec"], rec["tail"], rec["tail_count"])
    return prims, r


def host_buffer_entry(ob):
    prims, r = serial_recording(ob)
    return rendered(r, scenes.make_scene(prims))


def halton_bound(ob, integ, nsamples):
    """film_reference.bound of the Halton entry's film: what test_gpu_halton.py's test_two_batches_equal_one allows between two renders."""
    import film_reference as fr
    from test_halton_sampler import oracle_radiances, restated
    prims, r = c1(integ, nsamples)
    r.sampler = samplers(r)["halton"]()
    s = restated(r, [nsamples])
    Ls = oracle_radiances(ob, ob.OracleScene(prims), r, s)
    ref = fr.reference_from_samples(r.camera.film, s.pixel_xy, 1, s.vec[:, 0], s.vec[:, 1], Ls, serial=False)
    return fr.bound(ref.S, ref.n)


TWO_BATCH = ["ld64", "strat8x8"]


def two_batch_entry(which):
    """40 x 32 at 64 samples per pixel under BATCH_BITS = 16 (1024 pixels per batch): the smallest film of this width that makes two
    batches.  At 40 x 24 the window's 41 * 25 = 1025 pixels still go as ONE batch: planBatches lets a list of up to 5/4 of a batch's
    pixels do so (1280); 41 * 33 = 1353 pixels do not."""
    prims, r = c1("path", xres=40, yres=32, spp=64)
    if which == "strat8x8":
        r.sampler = core.StratifiedSampler(r.camera, 8, 8, True, 5489)
    scene = scenes.make_scene(prims)
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(b"BATCH_BITS", b"16"))
        return rendered(r, scene)
    finally:
        lib.dr_set_option(b"BATCH_BITS", None)


def _refusals():
    """name -> (renderer, scene prims, mutate(desc) or None, call(lib, handle, desc) or None): descriptors the library refuses."""
    def case(sampler, integ="all", nsamples=1, mutate=None, call=None):
        prims, r = c1(integ, nsamples)
        if sampler is not None:
            r.sampler = sampler(r) if callable(sampler) else samplers(r)[sampler]()
        return r, prims, mutate, call

    def dump(lib, h, d):
        out, px = np.zeros((4, 64), np.float32), np.zeros((4, 2), np.int32)
        return lib.dr_generate_samples(h, C.byref(d), px.ctypes.data, 4, out.ctypes.data, 64)

    def six_rows(r):
        return core.HostBufferSampler(r.camera, 1, np.zeros((6, 2), np.int32), np.full((6, 64), 0.5, np.float32))

    return {
        "ld_spp_3": case("ld", mutate=lambda d: setattr(d, "spp", 3)),
        "strat_xsamples_3_at_spp_4": case("strat", mutate=lambda d: setattr(d, "strat_xsamples", 3)),
        "strat_light_nsamples_3": case("strat", nsamples=3),
        "halton_light_nsamples_3": case("halton", nsamples=3),
        "halton_tile_count_2": case("halton", mutate=lambda d: setattr(d, "tile_count", 2)),
        "halton_spp_0": case("halton", mutate=lambda d: setattr(d, "spp", 0)),
        "adaptive_min_not_below_max": case("adaptive", mutate=lambda d: (setattr(d, "strat_xsamples", 8), setattr(d, "spp", 8))),
        "sampler_mode_99": case("ld", mutate=lambda d: setattr(d, "sampler_mode", 99)),
        "host_buffer_nsamples_not_a_multiple_of_spp": case(six_rows, mutate=lambda d: setattr(d, "spp", 4)),
        "generate_samples_in_halton_mode": case("halton", call=dump),
        "strat_spp_3_and_light_nsamples_3": case(lambda r: core.StratifiedSampler(r.camera, 3, 1, True, 5489), nsamples=3),  # two rules: which one wins
    }


REFUSALS = list(_refusals())


def refusal(name):
    """'<return code> <dr_last_error()>' of the refused descriptor `name`; the film must stay untouched."""
    r, prims, mutate, call = _refusals()[name]
    lib = _abi.lib()
    scene = scenes.make_scene(prims)
    d, keep = r.describe()
    if mutate:
        mutate(d)
    film = np.zeros((12, 16, 4), np.float32)
    h = scene._device().handle
    rc = call(lib, h, d) if call else lib.dr_render(h, C.byref(d), film.ctypes.data, None)
    assert rc != 0 and not film.any(), (name, rc)
    return "%d %s" % (rc, lib.dr_last_error().decode())


def mode_key(m):
    return "%s-%s" % (m[0], m[1])


def collect(ob):
    """Every stored array, as '<entry>/<field>'."""
    out = {}
    for m in MODES:
        out.update({"%s/%s" % (mode_key(m), k): v for k, v in mode_entry(*m).items()})
    out.update({"hostbuf-path/%s" % k: v for k, v in host_buffer_entry(ob).items()})
    for w in TWO_BATCH:
        out.update({"%s/%s" % (w, k): v for k, v in two_batch_entry(w).items()})
    for name in REFUSALS:
        out["refusal/" + name] = np.array(refusal(name))
    return out


def free_order(key):
    """The colour channels of a Halton film: compared within the stored bound, not bit for bit."""
    return key.startswith("halton-") and key.endswith("/film")


if __name__ == "__main__":
    import oracle.binding as ob
    _abi.init(0)
    first, second = collect(ob), collect(ob)
    for k, v in first.items():
        a, b = (v[..., 3], second[k][..., 3]) if free_order(k) else (v, second[k])
        if not np.array_equal(a, b):
            sys.exit("%s differs between two runs: not stored" % k)
    for m in MODES:
        if m[0] == "halton":
            first[mode_key(m) + "/film_bound"] = halton_bound(ob, m[1], m[2])
    np.savez_compressed(OUT, **first)
    for name in REFUSALS:
        print(name, "->", first["refusal/" + name])
    print("%d arrays, %d bytes" % (len(first), os.path.getsize(OUT)))
