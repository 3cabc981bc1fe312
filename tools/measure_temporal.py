"""The figures of MEASUREMENTS.md, "Temporal accumulation": the time of dr_temporal_device at 1024 x 1024 -- the second frame of a two-pose
sequence of BASELINE config C1, one degree apart, so that the history taps are a real gather -- beside dr_upsample_device (512^2 -> 1024^2,
2 x 2 taps) and dr_denoise_atrous_device at one and two levels, whose difference is one a-trous level, the yardstick.  HIP events on the
calls' own stream, warm-up calls dropped, the calls alternating within a round, one process.  Run from the repository root on a GPU; the
figures are printed, and written as JSON to OUT.json:

    python tools/measure_temporal.py OUT.json
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
prims, mk = scenes.config("C1", xres=W, yres=H, spp=4)
scene = scenes.make_scene(prims)
proto = mk()


def renderer(angle, seed):
    a = math.radians(angle)
    cam = core.PerspectiveCamera.lookAt((35.0 * math.sin(a), 0.0, -35.0 * math.cos(a)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0,
                                        core.ImageFilm(W, H, core.BoxFilter(0.5, 0.5)))
    return core.SamplerRenderer(core.LowDiscrepancySampler(cam, 4, seed), cam, proto.surfaceIntegrator, proto.volumeIntegrator)


pair = [renderer(0.0, 5489), renderer(1.0, 77)]
frames = denoise.render_sequence(pair, scene)
say("frames ready; history length 1 / 2 pixels of the second:", int((frames[1].len == 1).sum()), int((frames[1].len == 2).sum()))
res["pixels_len1_len2"] = [int((frames[1].len == 1).sum()), int((frames[1].len == 2).sum())]

up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
cur = [up(frames[1].noisy), up(frames[1].normal), up(frames[1].depth)]
hist = [up(frames[0].accumulated), up(frames[0].m2), up(frames[0].len), up(frames[0].normal), up(frames[0].depth)]
outs = [torch.empty((H, W, 3), device="cuda"), torch.empty((H, W), device="cuda"), torch.empty((H, W), device="cuda")]
low = [up(frames[1].noisy[::2, ::2]), up(frames[1].normal[::2, ::2]), up(frames[1].depth[::2, ::2])]
out3, scratch, stream = torch.empty((H, W, 3), device="cuda"), torch.empty(48 * W * H, dtype=torch.uint8, device="cuda"), torch.cuda.Stream()
torch.cuda.synchronize()
tp = denoise.temporal_params(denoise.temporal_matrices(pair[1].camera, pair[0].camera))
upp = denoise.upsample_params(2, 2)


def temporal_call():
    _abi.check(lib.dr_temporal_device(*[t.data_ptr() for t in cur], *[t.data_ptr() for t in hist], W, H, C.byref(tp), *[t.data_ptr() for t in outs],
                                      stream.cuda_stream))


def upsample_call():
    n = C.c_uint64(48 * W * H)
    _abi.check(lib.dr_upsample_device(low[0].data_ptr(), low[1].data_ptr(), low[2].data_ptr(), W // 2, H // 2, cur[1].data_ptr(), cur[2].data_ptr(),
                                      C.byref(upp), out3.data_ptr(), scratch.data_ptr(), C.byref(n), stream.cuda_stream))


def atrous_call(iterations):
    p = _abi.DrDenoiseParams(iterations, 1.0, 100.0, 1.0)

    def call():
        n = C.c_uint64(48 * W * H)
        _abi.check(lib.dr_denoise_atrous_device(cur[0].data_ptr(), cur[1].data_ptr(), cur[2].data_ptr(), W, H, C.byref(p), out3.data_ptr(),
                                                scratch.data_ptr(), C.byref(n), stream.cuda_stream))
    return call


calls = {"temporal": temporal_call, "upsample_f2_taps2": upsample_call, "atrous_1_level": atrous_call(1), "atrous_2_levels": atrous_call(2)}
res["time_ms"] = time_calls(calls, stream)
res["one_level_ms"] = res["time_ms"]["atrous_2_levels"]["median"] - res["time_ms"]["atrous_1_level"]["median"]
say(json.dumps(res["time_ms"]), "one a-trous level:", res["one_level_ms"])
# the device result equals the host's at this size too
temporal_call()
stream.synchronize()
host = denoise.temporal(frames[1].noisy, frames[1].normal, frames[1].depth, frames[0].history, denoise.temporal_matrices(pair[1].camera, pair[0].camera),
                        device=False)
res["bitwise_1024"] = bool(all(np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32)) for t, a in zip(outs, (host.rgb, host.m2, host.len))))
say("device == host at 1024 x 1024:", res["bitwise_1024"])
json.dump(res, open(OUT, "w"), indent=1)
say("measure_temporal: done")
