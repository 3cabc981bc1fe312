"""Times the Loop subdivision builders on one cage: the host builder (wall clock around dr_loop_subdivide) against the
device builder (the HIP-event time dr_loop_subdivide_device prints under DARTRAY_VERBOSE=2 -- every level, the limit positions and the
normals; uploads and the copy-out excluded -- and the wall clock of the whole call).  The cage is an icosahedron refined `--cage-levels`
times by the host builder and written out as a control mesh (5 levels: 20 480 faces).

    python tools/bench_subdiv.py --nlevels 4 [--cage-levels 5] [--repeat 3] [--builder both|host|device]
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["DARTRAY_VERBOSE"] = "2"

import numpy as np  # noqa: E402

from dartray_amd import _abi, core  # noqa: E402


def icosahedron():
    t = (1.0 + math.sqrt(5.0)) / 2.0
    P = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    return np.asarray(faces, np.uint32), np.asarray(P, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nlevels", type=int, default=4)
    ap.add_argument("--cage-levels", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--builder", default="both", choices=("both", "host", "device"))
    a = ap.parse_args()
    idx, P = icosahedron()
    P, _, idx, _ = core.loop_subdivide(idx, P, a.cage_levels, builder="host")
    print("cage: %d faces, %d vertices; nlevels %d -> %d faces" % (len(idx), len(P), a.nlevels, len(idx) * 4 ** a.nlevels), flush=True)
    out = {}
    if a.builder in ("both", "device"):
        _abi.init(0)
    for builder in ("host", "device"):
        if a.builder not in ("both", builder):
            continue
        for i in range(a.repeat):
            t0 = time.perf_counter()
            out[builder] = core.loop_subdivide(idx, P, a.nlevels, builder=builder)
            print("%s builder, run %d: %.1f ms wall (size query + refinement + copy-out)" % (builder, i, (time.perf_counter() - t0) * 1e3), flush=True)
    if len(out) == 2:
        same = all(np.array_equal(h.view(np.uint32), d.view(np.uint32)) for h, d in zip(out["host"][:3], out["device"][:3]))
        print("host and device outputs byte-identical: %s" % same)
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
