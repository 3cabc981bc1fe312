"""The figures of MEASUREMENTS.md, "Demodulation".

    python tools/measure_demodulate.py OUT.json [time|kernels|quality|all] [SIZE]

time     dr_demodulate_device and dr_remodulate_device with both images, and dr_firefly_device at radius 1 beside them, on one rendered
         SIZE x SIZE frame of BASELINE config C2 (default 1024): HIP events on the calls' own stream, warm-up calls dropped, the calls
         alternating within a round, one process (tools/measure_firefly.py's method).  Also the wall time of the two material renders and
         of a feature render ("depth") at 2 spp, each the median of five after a warm-up, with DrRenderStats.shade_ms of each.
kernels  the same device calls, enqueued 50 times each after a warm-up and nothing else: the run to put under the kernel trace, which
         gives the time of each KERNEL by name (k_demodulate, k_remodulate):
             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/measure_demodulate.py OUT.json kernels
quality  C2 at SIZE x SIZE against the 2048-spp render tools/measure_firefly.py uses: the mean squared error in unclipped radiance and on
         min(value, 1) for the plain filter, the pair filter and the moments filter (over 2 spp frames) at 2, 8 and 32 spp, each without
         demodulation, with the emission image alone, and with both images.  The chains are rebuilt from one set of renders with the
         module's own functions -- what render_denoised, render_denoised_pair and render_sequence compute with the keyword
         (tests/test_gpu_demodulate.py holds them to that) -- so that all arms see the same samples.

Run from the repository root on a GPU; the figures are printed, and written as JSON to OUT.json.
"""
import copy
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dartray_amd import _abi, core, denoise, scenes  # noqa: E402
from dartray_amd._image import _guides, _rerender  # noqa: E402

OUT = sys.argv[1]
MODE = sys.argv[2] if len(sys.argv) > 2 else "all"
SIZE = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
W = H = SIZE
WARMUP, ROUNDS = 10, 50
REF_SPP = 2048
ARMS = {"none": (), "emission": ("emission",), "both": ("emission", "albedo")}
res = json.load(open(OUT)) if os.path.exists(OUT) else {}
res["size"] = SIZE


def say(*a):
    print(*a, flush=True)


def save():
    json.dump(res, open(OUT, "w"), indent=1)


def stats(t):
    t = np.sort(np.array(t))
    return {"median": float(np.median(t)), "min": float(t[0]), "p10": float(t[len(t) // 10]), "p90": float(t[(9 * len(t)) // 10]), "max": float(t[-1])}


_abi.init(0)
lib = _abi.lib()
prims, mk = scenes.config("C2", xres=W, yres=H, spp=2)
scene = scenes.make_scene(prims)
say("built the scene")


def renderer(spp, seed=5489):
    proto = mk()
    return core.SamplerRenderer(core.LowDiscrepancySampler(proto.camera, spp, seed), proto.camera, proto.surfaceIntegrator, proto.volumeIntegrator)


def material(r, sampler=None):
    return {c: _rerender(r, scene, core.MaterialIntegrator(c), sampler).rgb for c in ("emission", "albedo")}


normal, depth = _guides(renderer(2), scene, "ns")
say("rendered the guides")


# ---- time ----
def device_calls():
    r = renderer(2)
    frame, mats = r.render(scene).rgb, material(r)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rgb, e, a, dn, dz = up(frame), up(mats["emission"]), up(mats["albedo"]), up(normal), up(depth)
    out, back, removed = torch.empty_like(rgb), torch.empty_like(rgb), torch.empty_like(dz)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    p, fp = denoise.demodulate_params(), denoise.firefly_params()
    calls = {
        "demodulate": lambda: _abi.check(lib.dr_demodulate_device(rgb.data_ptr(), e.data_ptr(), a.data_ptr(), W, H, C.byref(p), out.data_ptr(), stream.cuda_stream)),
        "remodulate": lambda: _abi.check(lib.dr_remodulate_device(out.data_ptr(), e.data_ptr(), a.data_ptr(), W, H, C.byref(p), back.data_ptr(), stream.cuda_stream)),
        "firefly_radius_1": lambda: _abi.check(lib.dr_firefly_device(rgb.data_ptr(), dn.data_ptr(), dz.data_ptr(), W, H, C.byref(fp), back.data_ptr(),
                                                                     removed.data_ptr(), stream.cuda_stream))}
    return calls, stream, [rgb, e, a, dn, dz, out, back, removed, p, fp], (frame, mats, out)


def time_calls(calls, stream):
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


def time_renders():
    out = {}
    r = renderer(2)
    for name, surface in (("material_emission", core.MaterialIntegrator("emission")), ("material_albedo", core.MaterialIntegrator("albedo")),
                          ("feature_depth", core.FeatureIntegrator("depth"))):
        rr = core.SamplerRenderer(r.sampler, r.camera, surface, r.volumeIntegrator)
        rr.render(scene)
        wall, shade = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            rr.render(scene)
            wall.append((time.perf_counter() - t0) * 1e3)
            shade.append(float(rr.last_stats["shade_ms"]))
        out[name] = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(min(wall)), "shade_ms_median": float(np.median(shade))}
    return out


if MODE in ("time", "all"):
    calls, stream, keep, (frame, mats, out) = device_calls()
    res["call_time_ms"] = time_calls(calls, stream)
    say(json.dumps(res["call_time_ms"]))
    calls["demodulate"]()
    stream.synchronize()
    want = denoise.demodulate(frame, mats["emission"], mats["albedo"], device=False)
    res["bitwise"] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)))
    say("device == host at %d x %d:" % (W, H), res["bitwise"])
    res["render_time_ms_2spp"] = time_renders()
    say(json.dumps(res["render_time_ms_2spp"]))
    save()

if MODE == "kernels":
    calls, stream, keep, _ = device_calls()
    for rounds in (WARMUP, ROUNDS):
        for _ in range(rounds):
            for fn in calls.values():
                fn()
        stream.synchronize()
    say("measure_demodulate: enqueued %d calls of each of %s" % (WARMUP + ROUNDS, ", ".join(calls)))


# ---- quality ----
def row(name, arm, img, ref):
    d = img.astype(np.float64) - ref
    dc = np.minimum(img.astype(np.float64), 1.0) - np.minimum(ref, 1.0)
    r = {"row": name, "demodulate": arm, "mse": float((d ** 2).mean()), "mse_clipped_at_1": float((dc ** 2).mean())}
    say(json.dumps(r))
    return r


def around(arm, mats, images, run):
    """run(demodulated images) remodulated: the chain of one arm over one set of renders."""
    e, a = (mats[c] if c in ARMS[arm] else None for c in ("emission", "albedo"))
    if arm == "none":
        return run(images)
    return denoise.remodulate(run([denoise.demodulate(x, e, a) for x in images]), e, a)


if MODE in ("quality", "all"):
    ref = renderer(REF_SPP).render(scene).rgb.astype(np.float64)
    say("rendered the reference at", REF_SPP, "spp")
    res["quality"] = []
    for spp in (2, 8, 32):
        rows = []
        r = renderer(spp)
        noisy, mats = r.render(scene).rgb, material(r)
        rows.append(row("unfiltered", "none", noisy, ref))
        for arm in ARMS:
            rows.append(row("plain_filter", arm, around(arm, mats, [noisy], lambda x: denoise.atrous(x[0], normal, depth)), ref))
        r = renderer(spp // 2)
        sampler_b = copy.copy(r.sampler)
        sampler_b.seed = denoise.pair_seed(r.sampler.seed)
        a, b, mats = r.render(scene).rgb, _rerender(r, scene, r.surfaceIntegrator, sampler_b).rgb, material(r)
        for arm in ARMS:
            rows.append(row("pair_filter", arm, around(arm, mats, [a, b], lambda x: denoise.atrous_pair(x[0], x[1], normal, depth)), ref))
        res["quality"].append({"spp": spp, "rows": rows})
        save()
    # the moments filter over static frames of 2 spp: 1, 4 and 16 frames are 2, 8 and 32 spp; one history per arm over the same renders
    cam_mats = denoise.temporal_matrices(mk().camera, mk().camera)
    hist, rows = {arm: None for arm in ARMS}, []
    for k in range(16):
        r = renderer(2, 5489 + 7919 * k)
        noisy, mats = r.render(scene).rgb, material(r)
        for arm in ARMS:
            e, a = (mats[c] if c in ARMS[arm] else None for c in ("emission", "albedo"))
            base = noisy if arm == "none" else denoise.demodulate(noisy, e, a)
            hist[arm] = denoise.temporal(base, normal, depth, hist[arm], cam_mats)
            if k + 1 in (1, 4, 16):
                mom = denoise.atrous_moments(hist[arm])
                rows.append(row("moments_filter_%d_spp" % (2 * (k + 1)), arm, mom if arm == "none" else denoise.remodulate(mom, e, a), ref))
        if k + 1 in (1, 4, 16):
            res["sequence"] = rows
            save()
say("measure_demodulate: done")
