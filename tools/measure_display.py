"""The figures of MEASUREMENTS.md, "The display transform": the time of dr_display_device at 1024 x 1024 with auto-exposure (histogram, pick,
encode) and with a manual exposure (encode alone), on a noise image and on an image of one luminance, for the library as built and for a
variant of dr_display_device.hip whose histogram kernel does not combine a wave's lanes before its LDS atomics.  HIP events on the call's
stream, 10 warm-up calls dropped, then 50 rounds that alternate every case.  From the repository root:

    python tools/measure_display.py --build-variant     # anywhere hipcc is: writes build/libdisplay_nocombine.so
    python tools/measure_display.py [OUT.json]          # on a GPU; prints the figures and writes them as JSON
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANT = os.path.join(ROOT, "build", "libdisplay_nocombine.so")


def build_variant():
    import __graft_entry__ as ge
    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    stub = os.path.join(os.path.dirname(VARIANT), "display_fail_stub.cpp")
    with open(stub, "w") as f:
        f.write('#include <string>\nstatic std::string g_error;\nint dr_fail(int code, const std::string& msg) {\n  g_error = msg;\n  return code;\n}\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    srcs = []
    for s in (os.path.join(ge.CSRC, "dr_display_device.hip"), os.path.join(ge.CSRC, "dr_display_host.cpp"), stub):
        srcs += ["-x", "hip", s]
    subprocess.check_call([hipcc] + ge.HIPCC_FLAGS + ["-DDR_DISPLAY_HIST_COMBINE=0", "-shared", "-o", VARIANT] + srcs)
    print("wrote", VARIANT)


if "--build-variant" in sys.argv:
    build_variant()
    raise SystemExit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dartray_amd import _abi, display  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
_abi.init(0)
libs = {"combine": _abi.lib()}
if os.path.exists(VARIANT):
    libs["no_combine"] = C.CDLL(VARIANT)
    libs["no_combine"].dr_display_device.argtypes = _abi.EXPORTS["dr_display_device"][1]
    libs["no_combine"].dr_display_device.restype = C.c_int

W = H = 1024
rng = np.random.Generator(np.random.PCG64(1))
images = {"noise": (10.0 ** rng.uniform(-3.0, 2.0, size=(H, W, 1)) * rng.uniform(0.2, 1.0, size=(H, W, 3))).astype(np.float32),
          "flat": np.full((H, W, 3), 0.42, np.float32)}
dev = {k: torch.from_numpy(v).cuda() for k, v in images.items()}
out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
NEED = 2048 * 4 + 16
scratch = torch.empty(NEED, dtype=torch.uint8, device="cuda")
stream = torch.cuda.Stream()
params = {"auto": display.params(), "manual": display.params(exposure=1.0)}
torch.cuda.synchronize()


def call(lib, image, mode):
    n = C.c_uint64(NEED)
    rc = lib.dr_display_device(dev[image].data_ptr(), W, H, C.byref(params[mode]), out.data_ptr(), scratch.data_ptr(), C.byref(n), stream.cuda_stream)
    if rc != 0:
        raise RuntimeError("dr_display_device: %d" % rc)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


cases = [(b, i, m) for b in libs for i in images for m in params]
for _ in range(10):
    for b, i, m in cases:
        call(libs[b], i, m)
stream.synchronize()
times = {c: [] for c in cases}
for _ in range(50):
    for c in cases:
        times[c].append(timed(lambda: call(libs[c[0]], c[1], c[2])))


def stats(t):
    t = np.sort(np.array(t))
    return {"median": float(np.median(t)), "min": float(t[0]), "p10": float(t[len(t) // 10]), "p90": float(t[(9 * len(t)) // 10]), "max": float(t[-1])}


res = {"time_ms": {"%s/%s/%s" % c: stats(t) for c, t in times.items()}}
for b in libs:
    for i in images:
        res["time_ms"]["%s/%s/auto_minus_manual" % (b, i)] = res["time_ms"]["%s/%s/auto" % (b, i)]["median"] - res["time_ms"]["%s/%s/manual" % (b, i)]["median"]
# the bytes agree with the host loop's at this size too, for both builds
res["bytes_equal_host"] = {}
for b in libs:
    for i in images:
        call(libs[b], i, "auto")
        stream.synchronize()
        res["bytes_equal_host"]["%s/%s" % (b, i)] = bool(np.array_equal(out.cpu().numpy(), display.tonemap(images[i], device=False)))
print(json.dumps(res, indent=1), flush=True)
if OUT:
    json.dump(res, open(OUT, "w"), indent=1)
print("measure_display: done")
