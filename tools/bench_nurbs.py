"""Times the NURBS builders on one bicubic patch: end to end through core.nurbs_dice for the host and the device builder
(wall clock, median of the repeats after a warm-up), and the kernels alone -- the HIP-event time dr_nurbs_dice_device prints to stderr
under DARTRAY_VERBOSE=2 (k_nurbs_dice and k_nurbs_indices; upload and copy-out excluded).

  python tools/bench_nurbs.py [--dice 30 1024] [--repeats 20]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dartray_amd import _abi, core  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dice", type=int, nargs="+", default=[30, 1024])
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    _abi.init(0)
    rng = np.random.RandomState(1)
    P = np.array([[3.0 * i / 3, 2.0 * j / 3, rng.uniform(-0.5, 0.5)] for j in range(4) for i in range(4)], np.float32)
    knots = [0, 0, 0, 0, 1, 1, 1, 1]
    for n in a.dice:
        for builder in ("host", "device"):
            times = []
            for r in range(a.repeats + 2):
                os.environ["DARTRAY_VERBOSE"] = "2" if r == a.repeats + 1 else "0"  # the last, untimed call prints the event time
                t0 = time.perf_counter()
                core.nurbs_dice(4, 4, knots, 0.25, 0.75, 4, 4, knots, 0.125, 0.5, P=P, diceu=n, dicev=n, builder=builder)
                if 0 < r <= a.repeats:
                    times.append(time.perf_counter() - t0)
            print("%4d x %-4d %-6s end to end: median %.3f ms, min %.3f ms over %d calls" % (n, n, builder, 1e3 * statistics.median(times),
                                                                                          1e3 * min(times), len(times)), flush=True)


if __name__ == "__main__":
    main()
