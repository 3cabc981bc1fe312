"""The figures of MEASUREMENTS.md, "Firefly suppression".

    python tools/measure_firefly.py OUT.json [time|kernels|quality|all] [SIZE]

time     dr_firefly_device at radius 1 and radius 2, dr_denoise_atrous_device at one level (k_image_pack + one k_denoise_level at step 1:
         25 taps served by L1) and dr_temporal_device with a history, on one rendered SIZE x SIZE frame of BASELINE config C2 (default
         1024): HIP events on the calls' own stream, warm-up calls dropped, the calls alternating within a round, one process.  These are
         CALL times; a call of the a-trous entry holds two kernels.
kernels  the same calls, enqueued 50 times each after a warm-up and nothing else: the run to put under the kernel trace, which gives the
         time of each KERNEL by name (k_firefly<1>, k_firefly<2>, k_denoise_level<DnRule>, k_image_pack, k_temporal):
             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/measure_firefly.py OUT.json kernels
quality  C2 at SIZE x SIZE against a 2048-spp render: the mean squared error in unclipped radiance and on min(value, 1), the share of
         pixels the stage clamped and the ratio of the mean luminance with the stage to that without, for the unfiltered render, the
         plain filter, the pair filter (the stage on each half) and the moments filter over 2, 8 and 32 static frames of 2 spp (the
         stage on each frame before it enters the history), each with and without the stage.  The chains are rebuilt from one set of
         renders with the module's own functions -- what render_denoised, render_denoised_pair and render_sequence compute with
         firefly=True (tests/test_gpu_firefly.py holds them to that) -- so that both arms see the same samples.

Run from the repository root on a GPU; the figures are printed, and written as JSON to OUT.json.
"""
import copy
import ctypes as C
import json
import os
import sys

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


normal, depth = _guides(renderer(2), scene, "ns")
say("rendered the guides")


# ---- time ----
def device_calls():
    frame = renderer(2).render(scene).rgb
    first = denoise.temporal(frame, normal, depth, None, denoise.temporal_matrices(mk().camera, mk().camera))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rgb, dn, dz, h_rgb, h_m2, h_len = up(frame), up(normal), up(depth), up(first.rgb), up(first.m2), up(first.len)
    out, removed, m2, ln = torch.empty_like(rgb), torch.empty_like(dz), torch.empty_like(dz), torch.empty_like(dz)
    scratch, stream = torch.empty(48 * W * H, dtype=torch.uint8, device="cuda"), torch.cuda.Stream()
    torch.cuda.synchronize()
    keep = [rgb, dn, dz, h_rgb, h_m2, h_len, out, removed, m2, ln, scratch]

    def firefly_call(radius):
        p = denoise.firefly_params(radius=radius)
        return lambda: _abi.check(lib.dr_firefly_device(rgb.data_ptr(), dn.data_ptr(), dz.data_ptr(), W, H, C.byref(p), out.data_ptr(),
                                                        removed.data_ptr(), stream.cuda_stream))

    def atrous_call():
        p, n = denoise.params(iterations=1), C.c_uint64(48 * W * H)
        _abi.check(lib.dr_denoise_atrous_device(rgb.data_ptr(), dn.data_ptr(), dz.data_ptr(), W, H, C.byref(p), out.data_ptr(), scratch.data_ptr(),
                                                C.byref(n), stream.cuda_stream))

    tp = denoise.temporal_params(denoise.temporal_matrices(mk().camera, mk().camera))

    def temporal_call():
        _abi.check(lib.dr_temporal_device(rgb.data_ptr(), dn.data_ptr(), dz.data_ptr(), h_rgb.data_ptr(), h_m2.data_ptr(), h_len.data_ptr(),
                                          dn.data_ptr(), dz.data_ptr(), W, H, C.byref(tp), out.data_ptr(), m2.data_ptr(), ln.data_ptr(),
                                          stream.cuda_stream))

    calls = {"firefly_radius_1": firefly_call(1), "firefly_radius_2": firefly_call(2), "atrous_1_level_pack_plus_step_1": atrous_call,
             "temporal_with_history": temporal_call}
    return calls, stream, keep, (frame, out, removed)


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


if MODE in ("time", "all"):
    calls, stream, keep, (frame, out, removed) = device_calls()
    res["call_time_ms"] = time_calls(calls, stream)
    say(json.dumps(res["call_time_ms"]))
    res["bitwise"] = {}
    for radius in (1, 2):                                                # the device result equals the host's at this size too
        calls["firefly_radius_%d" % radius]()
        stream.synchronize()
        want = denoise.firefly(frame, normal, depth, radius=radius, device=False, return_removed=True)
        res["bitwise"]["radius_%d" % radius] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
                                                    and np.array_equal(removed.cpu().numpy().view(np.uint32), want[1].view(np.uint32)))
    say("device == host at %d x %d:" % (W, H), res["bitwise"])
    save()

if MODE == "kernels":
    calls, stream, keep, _ = device_calls()
    for rounds in (WARMUP, ROUNDS):
        for _ in range(rounds):
            for fn in calls.values():
                fn()
        stream.synchronize()
    say("measure_firefly: enqueued %d calls of each of %s" % (WARMUP + ROUNDS, ", ".join(calls)))


# ---- quality ----
def lum(img):
    return img.astype(np.float64) @ np.array([0.212671, 0.715160, 0.072169])


def row(name, img, ref, base=None, removed=()):
    """One line of the table: the errors of `img`; with `base` (the same chain without the stage) the energy the stage cost."""
    d = img.astype(np.float64) - ref
    dc = np.minimum(img.astype(np.float64), 1.0) - np.minimum(ref, 1.0)
    r = {"row": name, "mse": float((d ** 2).mean()), "mse_clipped_at_1": float((dc ** 2).mean())}
    if base is not None:
        r["share_clamped"] = float(np.mean([(x != 0).mean() for x in removed]))
        r["mean_luminance_ratio"] = float(lum(img).mean() / lum(base).mean())
    say(json.dumps(r))
    return r


if MODE in ("quality", "all"):
    ref = renderer(REF_SPP).render(scene).rgb.astype(np.float64)
    say("rendered the reference at", REF_SPP, "spp")
    res["quality"] = []
    fire = lambda img: denoise.firefly(img, normal, depth, return_removed=True)
    for spp in (2, 8, 32):
        rows = []
        noisy = renderer(spp).render(scene).rgb
        clamped, removed = fire(noisy)
        rows.append(row("unfiltered", noisy, ref))
        rows.append(row("firefly_only", clamped, ref, noisy, [removed]))
        plain = denoise.atrous(noisy, normal, depth)
        rows.append(row("plain_filter", plain, ref))
        rows.append(row("plain_filter_with_stage", denoise.atrous(clamped, normal, depth), ref, plain, [removed]))
        r = renderer(spp // 2)
        sampler_b = copy.copy(r.sampler)
        sampler_b.seed = denoise.pair_seed(r.sampler.seed)
        a, b = r.render(scene).rgb, _rerender(r, scene, r.surfaceIntegrator, sampler_b).rgb
        (ca, ra), (cb, rb) = fire(a), fire(b)
        with np.errstate(all="ignore"):
            rows.append(row("mean_of_halves", np.float32(0.5) * (a + b), ref))
        pair = denoise.atrous_pair(a, b, normal, depth)
        rows.append(row("pair_filter", pair, ref))
        rows.append(row("pair_filter_with_stage", denoise.atrous_pair(ca, cb, normal, depth), ref, pair, [ra, rb]))
        res["quality"].append({"spp": spp, "rows": rows})
        save()
    # the moments filter over static frames of 2 spp: one history without the stage, one with it, over the same renders
    mats = denoise.temporal_matrices(mk().camera, mk().camera)
    hist, hist_c, removed_all, rows = None, None, [], []
    for k in range(32):
        noisy = renderer(2, 5489 + 7919 * k).render(scene).rgb
        clamped, removed = fire(noisy)
        removed_all.append(removed)
        hist = denoise.temporal(noisy, normal, depth, hist, mats)
        hist_c = denoise.temporal(clamped, normal, depth, hist_c, mats)
        if k + 1 in (2, 8, 32):
            rows.append(row("accumulated_%d_frames" % (k + 1), hist.rgb, ref))
            rows.append(row("accumulated_%d_frames_with_stage" % (k + 1), hist_c.rgb, ref, hist.rgb, removed_all))
            mom = denoise.atrous_moments(hist)
            rows.append(row("moments_filter_%d_frames" % (k + 1), mom, ref))
            rows.append(row("moments_filter_%d_frames_with_stage" % (k + 1), denoise.atrous_moments(hist_c), ref, mom, removed_all))
            res["sequence"] = rows
            save()
say("measure_firefly: done")
