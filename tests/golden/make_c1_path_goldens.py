"""Writes c1_path_counter.npz and c1_path_stratified.npz: C1 under PathIntegrator(5) on a 16 x 12 film as the frozen CPU oracle renders
it with the keyed low-discrepancy sampler (4 spp) and prices the restated stratified vectors (2 x 2, tests/stratified_restatement.py).
Depth 5 draws inside Li beyond the third vertex, so the two films pin the (pixel, sample) keys of the kind-2 streams of these modes
(tests/test_gpu_halton.py: the Halton sampler's own key must leave them alone).  Needs no GPU:  python tests/golden/make_c1_path_goldens.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import oracle.binding as ob  # noqa: E402
from dartray_amd import core, scenes  # noqa: E402
from test_stratified_sampler import oracle_film, window_pixels  # noqa: E402


def c1_path():
    prims, mk = scenes.config("C1", xres=16, yres=12, spp=4)
    r = mk()
    r.surfaceIntegrator = core.PathIntegrator(5)
    return prims, r


if __name__ == "__main__":
    prims, r = c1_path()
    osc = ob.OracleScene(prims)
    ref = osc.render(ob.render_desc(r, sampler_mode=1))
    np.savez(os.path.join(HERE, "c1_path_counter.npz"), film=ref["film"], rgb=ref["rgb"])
    r.sampler = core.StratifiedSampler(r.camera, 2, 2, True, 5489)
    film, rgb, _, _ = oracle_film(ob, osc, r, window_pixels(r), 2, 2, True, 5489, [1])
    np.savez(os.path.join(HERE, "c1_path_stratified.npz"), film=film, rgb=rgb)
    print("counter mean %.6f, stratified mean %.6f" % (ref["rgb"].mean(), rgb.mean()))
