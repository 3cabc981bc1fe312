"""The figures of MEASUREMENTS.md, "The pair denoiser": the time of dr_denoise_pair_device against dr_denoise_atrous_device in one process
(1024 x 1024, five levels, HIP events on the call's stream, alternating), and on the C2 BASELINE scene the RMSE against a 2048-spp render of the
unfiltered image and render_denoised at 2N samples per pixel and of render_denoised_pair at N + N, for N = 2, 8, 32.  Run from the repository
root on a GPU; the figures are printed, and written as JSON to the file named by the first argument, if any:

    python tools/measure_denoise_pair.py [OUT.json]
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dartray_amd import _abi, core, denoise, scenes  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
res = {}
_abi.init(0)
lib = _abi.lib()


def say(*a):
    print(*a, flush=True)


def save():
    if OUT:
        json.dump(res, open(OUT, "w"), indent=1)


# ---- time ----
W = H = 1024
prims, mk = scenes.config("C2", xres=W, yres=H, spp=4)
scene = scenes.make_scene(prims)
pair = denoise.render_denoised_pair(mk(), scene)
say("rendered the 4 + 4 spp pair")
a, b, normal, depth = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (pair.a, pair.b, pair.normal, pair.depth))
out, var = torch.empty_like(a), torch.empty_like(depth)
scratch = torch.empty(48 * W * H, dtype=torch.uint8, device="cuda")
stream = torch.cuda.Stream()
pp, pl = denoise.pair_params(), denoise.params()
torch.cuda.synchronize()


def call_pair(v=True):
    n = C.c_uint64(48 * W * H)
    _abi.check(lib.dr_denoise_pair_device(a.data_ptr(), b.data_ptr(), normal.data_ptr(), depth.data_ptr(), W, H, C.byref(pp), out.data_ptr(),
                                          var.data_ptr() if v else None, scratch.data_ptr(), C.byref(n), stream.cuda_stream))


def call_plain():
    n = C.c_uint64(48 * W * H)
    _abi.check(lib.dr_denoise_atrous_device(a.data_ptr(), normal.data_ptr(), depth.data_ptr(), W, H, C.byref(pl), out.data_ptr(),
                                            scratch.data_ptr(), C.byref(n), stream.cuda_stream))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


for _ in range(10):
    call_pair()
    call_plain()
stream.synchronize()
tp, tq, tl = [], [], []
for _ in range(50):                                                     # alternating
    tp.append(timed(call_pair))
    tl.append(timed(call_plain))
    tq.append(timed(lambda: call_pair(False)))


def stats(t):
    t = np.sort(np.array(t))
    return {"median": float(np.median(t)), "min": float(t[0]), "p10": float(t[len(t) // 10]), "p90": float(t[(9 * len(t)) // 10]), "max": float(t[-1])}


res["time_ms"] = {"pair": stats(tp), "pair_no_variance_output": stats(tq), "plain": stats(tl)}
res["time_ms"]["ratio_of_medians"] = res["time_ms"]["pair"]["median"] / res["time_ms"]["plain"]["median"]
say(json.dumps(res["time_ms"]))
# the device result equals the host's at this size too
call_pair()
stream.synchronize()
h_out, h_var = denoise.atrous_pair(pair.a, pair.b, pair.normal, pair.depth, device=False, return_variance=True)
res["bitwise_1024"] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), h_out.view(np.uint32))
                           and np.array_equal(var.cpu().numpy().view(np.uint32), h_var.view(np.uint32))
                           and np.array_equal(pair.rgb.view(np.uint32), h_out.view(np.uint32)))
say("device == host at 1024 x 1024:", res["bitwise_1024"])
save()

# ---- quality ----
REF_SPP = 2048
_, mk_ref = scenes.config("C2", xres=W, yres=H, spp=REF_SPP)
ref = mk_ref().render(scene).rgb.astype(np.float64)
say("rendered the reference at", REF_SPP, "spp")


def rmse(img):
    return float(np.sqrt(((img.astype(np.float64) - ref) ** 2).mean()))


def rmse_clipped(img):
    """The same on min(value, 1): what a display shows; takes the emitter's and the fireflies' weight out of the figure."""
    return float(np.sqrt(((np.minimum(img.astype(np.float64), 1.0) - np.minimum(ref, 1.0)) ** 2).mean()))


res["quality"] = []
for n in (2, 8, 32):
    _, mk_full = scenes.config("C2", xres=W, yres=H, spp=2 * n)
    _, mk_half = scenes.config("C2", xres=W, yres=H, spp=n)
    plain = denoise.render_denoised(mk_full(), scene)
    pr_ = denoise.render_denoised_pair(mk_half(), scene)
    row = {"N": n}
    for name, img in (("unfiltered_2N", plain.noisy), ("plain_filter_2N", plain.rgb), ("mean_of_N_plus_N", pr_.noisy), ("pair_filter_N_plus_N", pr_.rgb)):
        row[name] = {"rmse": rmse(img), "rmse_clipped_at_1": rmse_clipped(img)}
    row["valid_fraction"] = float((pr_.variance >= 0).mean())
    row["median_variance_in"] = float(np.median(0.25 * ((pr_.a - pr_.b).astype(np.float64) @ np.array([0.212671, 0.715160, 0.072169])) ** 2))
    row["median_variance_out"] = float(np.median(pr_.variance))
    res["quality"].append(row)
    say(json.dumps(row))
save()
say("pair_measure: done")
