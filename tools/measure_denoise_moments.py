"""The figures of MEASUREMENTS.md, "The moments denoiser".

Time: dr_denoise_moments_device at 1024 x 1024 and five levels on three history-length fields over one rendered frame -- long everywhere (no
spatial gather), one pixel in seven short (scattered: every wave diverges), and the same share as vertical bands (what a disocclusion looks
like) -- beside dr_denoise_pair_device on the same colour and guides, and both at one level, so that the difference is the estimate pass.
HIP events on the calls' own stream, warm-up calls dropped, the calls alternating within a round, one process.

Quality: BASELINE config C2 (blob at 250 x 125) at 256 x 256 and 2 samples per pixel per frame: a static camera over 2, 8 and 32 frames and an
eight-frame orbit, one degree per frame; the RMSE against a 1024-spp render of the last pose of the accumulated image alone, of
render_sequence(denoise=True) and of render_sequence(denoise="moments"), on unclipped radiance and on min(value, 1).

Run from the repository root on a GPU; the figures are printed, and written as JSON to OUT.json:

    python tools/measure_denoise_moments.py OUT.json
"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dartray_amd import _abi, core, denoise, scenes  # noqa: E402

OUT = sys.argv[1]
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


_abi.init(0)
lib = _abi.lib()
BLOB = (250, 125)

# ---- time ----
prims, mk = scenes.config("C2", xres=W, yres=H, spp=4, blob=BLOB)
scene = scenes.make_scene(prims)
frame = denoise.render_sequence([mk()], scene)[0]
say("rendered the 1024 x 1024 frame")
lum = frame.history.rgb @ np.array([0.212671, 0.715160, 0.072169], np.float32)
m2 = (lum * lum * np.float32(1.25)).astype(np.float32)                  # a variance of a quarter of lum^2 per frame
x, y = np.meshgrid(np.arange(W), np.arange(H))
fields = {"long": np.full((H, W), 32.0, np.float32),
          "scattered_1_in_7": np.where((x + 3 * y) % 7 == 0, 1.0, 32.0).astype(np.float32),
          "bands_1_in_7": np.where(x % 448 < 64, 1.0, 32.0).astype(np.float32)}
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
rgb, dm2, normal, depth = up(frame.history.rgb), up(m2), up(frame.normal), up(frame.depth)
lens = {k: up(v) for k, v in fields.items()}
out, var, var0 = torch.empty_like(rgb), torch.empty_like(depth), torch.empty_like(depth)
scratch, stream = torch.empty(48 * W * H, dtype=torch.uint8, device="cuda"), torch.cuda.Stream()
torch.cuda.synchronize()


def moments_call(field, iterations):
    p = denoise.moments_params(iterations=iterations)

    def call():
        n = C.c_uint64(48 * W * H)
        _abi.check(lib.dr_denoise_moments_device(rgb.data_ptr(), dm2.data_ptr(), lens[field].data_ptr(), normal.data_ptr(), depth.data_ptr(), W, H,
                                                 C.byref(p), out.data_ptr(), var.data_ptr(), var0.data_ptr(), scratch.data_ptr(), C.byref(n),
                                                 stream.cuda_stream))
    return call


def pair_call(iterations):
    p = denoise.pair_params(iterations=iterations)

    def call():
        n = C.c_uint64(48 * W * H)
        _abi.check(lib.dr_denoise_pair_device(rgb.data_ptr(), rgb.data_ptr(), normal.data_ptr(), depth.data_ptr(), W, H, C.byref(p), out.data_ptr(),
                                              var.data_ptr(), scratch.data_ptr(), C.byref(n), stream.cuda_stream))
    return call


def plain_call():
    p = denoise.params()
    n = C.c_uint64(48 * W * H)
    _abi.check(lib.dr_denoise_atrous_device(rgb.data_ptr(), normal.data_ptr(), depth.data_ptr(), W, H, C.byref(p), out.data_ptr(), scratch.data_ptr(),
                                            C.byref(n), stream.cuda_stream))


calls = {"pair_5_levels": pair_call(5), "pair_1_level": pair_call(1), "plain_5_levels": plain_call}
for k in fields:
    calls["moments_5_levels_" + k] = moments_call(k, 5)
    calls["moments_1_level_" + k] = moments_call(k, 1)
res["short_history_share"] = {k: float((v < 4).mean()) for k, v in fields.items()}
res["time_ms"] = t = time_calls(calls, stream)
res["estimate_pass_ms"] = {k: {"at_5_levels": t["moments_5_levels_" + k]["median"] - t["pair_5_levels"]["median"],
                               "at_1_level": t["moments_1_level_" + k]["median"] - t["pair_1_level"]["median"]} for k in fields}
say(json.dumps(res["time_ms"]))
say("the estimate pass (stage minus pair filter, medians):", json.dumps(res["estimate_pass_ms"]))
# the device result equals the host's at this size too
res["bitwise_1024"] = {}
for k in fields:
    moments_call(k, 5)()
    stream.synchronize()
    want = denoise.atrous_moments(denoise.TemporalFrame(frame.history.rgb, m2, fields[k], frame.normal, frame.depth), device=False,
                                  return_variance=True, return_estimate=True)
    res["bitwise_1024"][k] = bool(all(np.array_equal(t_.cpu().numpy().view(np.uint32), a.view(np.uint32)) for t_, a in zip((out, var, var0), want)))
say("device == host at 1024 x 1024:", res["bitwise_1024"])
save()

# ---- quality ----
Q, SPP, REF_SPP = 256, 2, 1024
prims, mk = scenes.config("C2", xres=Q, yres=Q, spp=SPP, blob=BLOB)
proto = mk()


def renderer(angle, seed, spp=SPP):
    a = math.radians(angle)
    cam = core.PerspectiveCamera.lookAt((35.0 * math.sin(a), 0.0, -35.0 * math.cos(a)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0,
                                        core.ImageFilm(Q, Q, core.BoxFilter(0.5, 0.5)))
    return core.SamplerRenderer(core.LowDiscrepancySampler(cam, spp, seed), cam, proto.surfaceIntegrator, proto.volumeIntegrator)


def errors(img, ref):
    d = img.astype(np.float64) - ref
    dc = np.minimum(img.astype(np.float64), 1.0) - np.minimum(ref, 1.0)
    return {"rmse": float(np.sqrt((d ** 2).mean())), "rmse_clipped_at_1": float(np.sqrt((dc ** 2).mean()))}


refs = {}
res["quality"] = []
runs = [("static", n, [0.0] * n) for n in (2, 8, 32)] + [("orbit_1_degree_per_frame", 8, [float(k) for k in range(8)])]
for name, n, angles in runs:
    if angles[-1] not in refs:
        refs[angles[-1]] = renderer(angles[-1], 5489, REF_SPP).render(scene).rgb.astype(np.float64)
        say("rendered the reference at", angles[-1], "degrees")
    ref = refs[angles[-1]]
    rs = [renderer(a, 5489 + 7919 * k) for k, a in enumerate(angles)]
    plain = denoise.render_sequence(rs, scene, denoise=True)[-1]
    mom = denoise.render_sequence(rs, scene, denoise="moments")[-1]
    assert np.array_equal(plain.accumulated.view(np.uint32), mom.accumulated.view(np.uint32))
    est = denoise.atrous_moments(mom.history, return_estimate=True)[1]
    row = {"run": name, "frames": n, "last_frame_alone": errors(mom.noisy, ref), "accumulated": errors(mom.accumulated, ref),
           "plain_filter": errors(plain.rgb, ref), "moments_filter": errors(mom.rgb, ref),
           "share_len_below_4": float((mom.len < 4).mean()), "valid_fraction": float((est >= 0).mean()),
           "median_estimate": float(np.median(est[est >= 0])), "median_filtered_variance": float(np.median(mom.filtered_variance[est >= 0]))}
    res["quality"].append(row)
    say(json.dumps(row))
    save()
say("measure_denoise_moments: done")
