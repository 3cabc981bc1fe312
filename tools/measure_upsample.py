"""The figures of MEASUREMENTS.md, "The upsampler": the time of dr_upsample_device at 512^2 -> 1024^2 and 256^2 -> 1024^2 with 2 x 2 and 4 x 4
taps beside dr_denoise_atrous_device at one, two and five levels (HIP events on the call's stream, alternating, one process), and on the C2
BASELINE scene at 1024 x 1024 the wall time of the full render and of render_upsampled at factor 2 and 4 at equal samples per pixel, with the
RMSE of each against a 2048-spp render.  Run from the repository root on a GPU; the figures are printed, and written as JSON to OUT.json:

    python tools/measure_upsample.py OUT.json [INPUTS.npz]          everything; INPUTS.npz: the a-trous timing's inputs are kept there
    python tools/measure_upsample.py OUT.json INPUTS.npz LIB.so     only the a-trous timing, on another build of the library (an A/B run)
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dartray_amd import _abi  # noqa: E402

OUT = sys.argv[1]
INPUTS = sys.argv[2] if len(sys.argv) > 2 else None
OTHER_LIB = sys.argv[3] if len(sys.argv) > 3 else None
W = H = 1024
WARMUP, ROUNDS = 10, 50
res = {}


def say(*a):
    print(*a, flush=True)


def save():
    json.dump(res, open(OUT, "w"), indent=1)


def stats(t):
    t = np.sort(np.array(t))
    return {"median": float(np.median(t)), "min": float(t[0]), "p10": float(t[len(t) // 10]), "p90": float(t[(9 * len(t)) // 10]), "max": float(t[-1])}


def time_calls(calls, stream):
    """{name: stats of ROUNDS timed calls} for {name: function that enqueues one call on `stream`}, the calls alternating within a round."""
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(WARMUP):
        for fn in calls.values():
            fn()
    stream.synchronize()
    t = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            t[k].append(timed(fn))
    return {k: stats(v) for k, v in t.items()}


def atrous_calls(lib, rgb, normal, depth, out, scratch, stream, check):
    def one(iterations):
        p = _abi.DrDenoiseParams(iterations, 1.0, 100.0, 1.0)

        def call():
            n = C.c_uint64(48 * W * H)
            check(lib.dr_denoise_atrous_device(rgb.data_ptr(), normal.data_ptr(), depth.data_ptr(), W, H, C.byref(p), out.data_ptr(), scratch.data_ptr(),
                                               C.byref(n), stream.cuda_stream))
        return call
    return {"atrous_%d_level%s" % (i, "s" if i > 1 else ""): one(i) for i in (1, 2, 5)}


if OTHER_LIB:                                                           # the A/B run: another build's a-trous kernels on the kept inputs
    _abi._share_hip_runtime_with_torch()
    lib = C.CDLL(OTHER_LIB)
    lib.dr_last_error.restype = C.c_char_p
    lib.dr_denoise_atrous_device.argtypes = _abi.EXPORTS["dr_denoise_atrous_device"][1]

    def check(rc):
        if rc != 0:
            raise RuntimeError(lib.dr_last_error().decode())
    check(lib.dr_init(0))
    z = np.load(INPUTS)
    rgb, normal, depth = (torch.from_numpy(z[k]).cuda() for k in ("rgb", "normal", "depth"))
    out, scratch, stream = torch.empty_like(rgb), torch.empty(48 * W * H, dtype=torch.uint8, device="cuda"), torch.cuda.Stream()
    torch.cuda.synchronize()
    res["library"] = OTHER_LIB
    res["time_ms"] = time_calls(atrous_calls(lib, rgb, normal, depth, out, scratch, stream, check), stream)
    t = res["time_ms"]
    res["one_level_ms"] = t["atrous_2_levels"]["median"] - t["atrous_1_level"]["median"]
    say(json.dumps(res))
    save()
    sys.exit(0)

from dartray_amd import denoise, scenes  # noqa: E402

_abi.init(0)
lib = _abi.lib()
SPP = (4, 16, 64)
prims, mk4 = scenes.config("C2", xres=W, yres=H, spp=4)
scene = scenes.make_scene(prims)


def renderer(res_, spp):
    return scenes.config("C2", xres=res_, yres=res_, spp=spp)[1]()


mk4().render(scene)                                                     # the scene's first big render measures its kernels: not timed
say("scene ready")

# ---- kernel time ----
ups = {f: denoise.render_upsampled(renderer(W // f, 4), renderer(W, 4), scene) for f in (2, 4)}
normal, depth = (torch.from_numpy(a).cuda() for a in (ups[2].normal, ups[2].depth))
lows = {f: [torch.from_numpy(a).cuda() for a in (ups[f].low, ups[f].normal_lo, ups[f].depth_lo)] for f in (2, 4)}
rgb = torch.from_numpy(ups[2].rgb).cuda()
out, scratch, stream = torch.empty_like(normal), torch.empty(48 * W * H, dtype=torch.uint8, device="cuda"), torch.cuda.Stream()
torch.cuda.synchronize()


def upsample_call(f, taps):
    p = denoise.upsample_params(f, taps)
    lo = lows[f]

    def call():
        n = C.c_uint64(48 * W * H)
        _abi.check(lib.dr_upsample_device(lo[0].data_ptr(), lo[1].data_ptr(), lo[2].data_ptr(), W // f, H // f, normal.data_ptr(), depth.data_ptr(),
                                          C.byref(p), out.data_ptr(), scratch.data_ptr(), C.byref(n), stream.cuda_stream))
    return call


calls = {"upsample_f%d_taps%d" % (f, t): upsample_call(f, t) for f in (2, 4) for t in (2, 4)}
calls.update(atrous_calls(lib, rgb, normal, depth, out, scratch, stream, _abi.check))
res["time_ms"] = time_calls(calls, stream)
res["one_level_ms"] = res["time_ms"]["atrous_2_levels"]["median"] - res["time_ms"]["atrous_1_level"]["median"]
say(json.dumps(res["time_ms"]), "one a-trous level:", res["one_level_ms"])
# the device result equals the host's at this size too
res["bitwise_1024"] = {}
for f in (2, 4):
    upsample_call(f, 2)()
    stream.synchronize()
    host = denoise.upsample(ups[f].low, ups[f].normal_lo, ups[f].depth_lo, ups[f].normal, ups[f].depth, device=False)
    res["bitwise_1024"]["f%d" % f] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), host.view(np.uint32))
                                          and np.array_equal(ups[f].rgb.view(np.uint32), host.view(np.uint32)))
say("device == host at 1024 x 1024:", res["bitwise_1024"])
if INPUTS:
    np.savez(INPUTS, rgb=ups[2].rgb, normal=ups[2].normal, depth=ups[2].depth)
save()

# ---- saving and cost ----
REF_SPP = 2048
ref = renderer(W, REF_SPP).render(scene).rgb.astype(np.float64)
say("rendered the reference at", REF_SPP, "spp")


def rmse(img):
    return float(np.sqrt(((img.astype(np.float64) - ref) ** 2).mean()))


def rmse_clipped(img):
    """The same on min(value, 1): what a display shows; takes the emitter's and the fireflies' weight out of the figure."""
    return float(np.sqrt(((np.minimum(img.astype(np.float64), 1.0) - np.minimum(ref, 1.0)) ** 2).mean()))


def wall(fn, n=5):
    """(median wall seconds of n calls after one that is dropped, the last result); every call ends with the image on the host."""
    fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        r = fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), r


res["render"] = []
for spp in SPP:
    row = {"spp": spp}
    full = renderer(W, spp)
    jobs = [("full_render", lambda: full.render(scene)), ("render_denoised", lambda: denoise.render_denoised(full, scene))]
    for f in (2, 4):
        low = renderer(W // f, spp)
        jobs.append(("upsampled_f%d" % f, lambda low=low: denoise.render_upsampled(low, full, scene)))
        jobs.append(("upsampled_f%d_taps4" % f, lambda low=low: denoise.render_upsampled(low, full, scene, taps=4)))
        jobs.append(("upsampled_f%d_denoised" % f, lambda low=low: denoise.render_upsampled(low, full, scene, denoise=True)))
        jobs.append(("low_render_f%d_alone" % f, lambda low=low: low.render(scene)))
    jobs.append(("guides_1024_alone", lambda: (denoise.SamplerRenderer(full.sampler, full.camera, denoise.FeatureIntegrator("ns"), full.volumeIntegrator).render(scene),
                                               denoise.SamplerRenderer(full.sampler, full.camera, denoise.FeatureIntegrator("depth"), full.volumeIntegrator).render(scene))))
    for name, fn in jobs:
        seconds, r = wall(fn)
        row[name] = {"wall_ms": 1000.0 * seconds}
        if hasattr(r, "rgb") and r.rgb.shape == (H, W, 3):
            row[name].update(rmse=rmse(r.rgb), rmse_clipped_at_1=rmse_clipped(r.rgb))
    res["render"].append(row)
    say(json.dumps(row))
    save()
say("measure_upsample: done")
