"""Rays that land inside the band of the traversal kernels' f32 slab filter, on purpose (inputs and a restatement; no GPU).

dr_trace.hip decides almost every box with an f32 enclosure of the slab test (slab_f32_sure / slab_bounds: every f32 parameter
+-(|x| * 2^-21 + 1e-37)) and promises that "the decision is therefore always the f64 one".  Random rays meet the band by accident
only.  This module restates the literal test (slab_f64) and the filter (slab_f32_sure) in numpy -- every f32 operation in
np.float32, the fused |x| * R + A in f64 rounded once (exact: R is a power of two) -- and builds rays, from the oracle's node array,
whose entry / exit parameters at a chosen box differ from each other, from maxDistance or from minDistance by rounding only.
The restatement belongs to the tests: it says which rays are in the band and checks the constants; the oracle stays the reference
for every hit and counter.

Families (band_family): edge, tmax, tmin, facehit on band_prims(); tiny / huge = edge + tmax + tmin on band_prims(2^-100) /
band_prims(2^40).  Every ray is finite and has no zero direction component (a zero component sends a ray past the filter).
"""
import functools

import numpy as np

from dartray_amd import core, scenes

F32, F64 = np.float32, np.float64
R_FILTER = 2.0 ** -21                 # slab_f32_sure / slab_bounds / pruneStack / popNext: R
A_FILTER = float(np.float32(1.0e-37))  # ... and A (the f32 constant 1.0e-37f)
FAMILIES = ("edge", "tmax", "tmin", "facehit", "tiny", "huge")
SCALES = {"edge": 1.0, "tmax": 1.0, "tmin": 1.0, "facehit": 1.0, "tiny": 2.0 ** -100, "huge": 2.0 ** 40}


# ---------------------------------------------------------------------------
# restatement
# ---------------------------------------------------------------------------
def inv_dir(d):
    """invDir is a Vector: 1 / d in f64, rounded to f32 (bvh_accel.dart:109-111; ray_init)."""
    return (1.0 / np.asarray(d, F32).astype(F64)).astype(F32)


def f32_below(v):
    """Largest f32 <= v (f32_below)."""
    v = np.asarray(v, F64)
    f = v.astype(F32)
    return np.where(f.astype(F64) > v, np.nextafter(f, F32(-np.inf)), f).astype(F32)


def f32_above(v):
    """Smallest f32 >= v (f32_above)."""
    v = np.asarray(v, F64)
    f = v.astype(F32)
    return np.where(f.astype(F64) < v, np.nextafter(f, F32(np.inf)), f).astype(F32)


def slab_f64(o, d, tmin, tmax, bmin, bmax):
    """The literal slab test (bvh_accel.dart:439-472; slab_f64), one box per ray.  Returns (hit, geom, E, X): geom = neither early
    return was taken, E / X = the entry / exit parameter the last line compares with maxDistance / minDistance."""
    iv32 = inv_dir(d)
    neg = iv32 < 0
    iv, o = iv32.astype(F64), np.asarray(o, F32).astype(F64)
    bmin, bmax = np.asarray(bmin, F32), np.asarray(bmax, F32)
    tn = (np.where(neg, bmax, bmin).astype(F64) - o) * iv
    tf = (np.where(neg, bmin, bmax).astype(F64) - o) * iv
    t0, t1 = tn[:, 0], tf[:, 0]
    geom = ~((t0 > tf[:, 1]) | (tn[:, 1] > t1))
    t0 = np.where(tn[:, 1] > t0, tn[:, 1], t0)
    t1 = np.where(tf[:, 1] < t1, tf[:, 1], t1)
    geom &= ~((t0 > tf[:, 2]) | (tn[:, 2] > t1))
    t0 = np.where(tn[:, 2] > t0, tn[:, 2], t0)
    t1 = np.where(tf[:, 2] < t1, tf[:, 2], t1)
    return geom & (t0 < tmax) & (t1 > tmin), geom, t0, t1


def slab_f32_sure(o, d, tmin, tmax, bmin, bmax, R=R_FILTER, A=A_FILTER):
    """The f32 filter (slab_f32_sure), one box per ray.  Returns (sureHit, sureMiss); neither = ambiguous, the literal test decides."""
    o, iv = np.asarray(o, F32), inv_dir(d)
    with np.errstate(over="ignore", invalid="ignore"):
        a = (np.asarray(bmin, F32) - o) * iv
        b = (np.asarray(bmax, F32) - o) * iv
        mn, mx = np.minimum(a, b), np.maximum(a, b)
        lo = np.maximum(np.maximum(mn[:, 0], mn[:, 1]), mn[:, 2])
        hi = np.minimum(np.minimum(mx[:, 0], mx[:, 1]), mx[:, 2])
        eLo = (np.abs(lo).astype(F64) * R + A).astype(F32)  # v_fma_f32 |lo|, R, A: one rounding
        eHi = (np.abs(hi).astype(F64) * R + A).astype(F32)
        loU, loL, hiU, hiL = lo + eLo, lo - eLo, hi + eHi, hi - eHi
        tmaxHi, tminLo = f32_above(tmax), f32_below(tmin)
        sureHit = (loU <= hiL) & (loU < tmaxHi) & (hiL > tminLo)
        sureMiss = (loL > hiU) | (loL >= tmaxHi) | (hiU <= tminLo)
    assert loU.dtype == F32 and hiL.dtype == F32
    return sureHit, sureMiss


# ---------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------
CHAIN_N, CHAIN_RATIO = 60, 4.0  # as in test_deep_tree_uses_the_spill_stack: coordinates up to 2^118
CHAIN_N_SCALED = 12               # the scaled copies keep the first 12 triangles (up to 2^22): times 2^40 the products of two
                                  # coordinates in Triangle.intersectP's f32 temporaries stay below 2^128 -- nothing overflows


def chain_mesh(n, ratio, scale=1.0):
    """The geometric progression of tests/test_gpu_intersect.py::test_deep_tree_uses_the_spill_stack: triangle k in the plane
    x = ratio^k, 0.3 ratio^k wide: the SAH tree is one long chain."""
    s = float(ratio) ** np.arange(n)
    P = np.zeros((n, 3, 3), F64)
    P[:, 0] = np.stack([s, 0 * s, 0 * s], 1)
    P[:, 1] = np.stack([s, 0.3 * s, 0 * s], 1)
    P[:, 2] = np.stack([s, 0 * s, 0.3 * s], 1)
    return core.TriangleMesh(np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), (P.reshape(-1, 3).astype(F32) * F32(scale)).astype(F32))


def shingle_mesh(scale=1.0):
    """The shingle stack: 10 planes y = -1 + k / 4 of four unit quads each, a row along x whose neighbours share an edge (their flat
    leaf boxes share a face), every plane staggered by half a quad in x and a quarter in z against the one below -- so a quad lies in
    the top or bottom face of the boxes that group quads of the planes next to it.  Every seventh quad is tilted by 1/16 (its two
    triangles then have boxes of their own, not flat).  All coordinates are multiples of 1/16: coincident planes coincide exactly."""
    P, idx = [], []
    q = 0
    for k in range(10):
        y = -1.0 + 0.25 * k
        x0 = -16.0 + 0.5 * (k % 2)
        z0 = 2.0 + 0.25 * (k % 4)
        for i in range(4):
            lift = 0.0625 if q % 7 == 3 else 0.0
            base = len(P)
            P += [(x0 + i, y, z0), (x0 + i + 1, y, z0), (x0 + i + 1, y + lift, z0 + 1), (x0 + i, y + lift, z0 + 1)]
            idx += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
            q += 1
    return core.TriangleMesh(np.array(idx, np.uint32), (np.array(P, F32) * F32(scale)).astype(F32))


SHINGLE_MESH = 0  # index of the shingle stack among band_prims(): OracleScene.bvh()'s `mesh` column names it


def band_prims(scale=1.0):
    """Shingle stack + a small blob (ordinary leaves) + the chain (a tree deeper than 32) + the Cornell emitter, all vertices times
    `scale` (a power of two: exact, but for coordinates that fall below the f32 normal range at 2^-100).  A scaled copy has the
    short chain (CHAIN_N_SCALED)."""
    grey = core.MatteMaterial((0.5, 0.5, 0.5))
    blob = scenes.blob_mesh(16, 8)
    em = scenes.emitter_quad()
    scaled = lambda m: core.TriangleMesh(m.vertexIndex, (np.asarray(m.P, F32) * F32(scale)).astype(F32))
    return [core.GeometricPrimitive(shingle_mesh(scale), core.MatteMaterial((0.6, 0.5, 0.4))),
            core.GeometricPrimitive(scaled(blob), core.MatteMaterial((0.48, 0.48, 0.48))),
            core.GeometricPrimitive(chain_mesh(CHAIN_N if scale == 1.0 else CHAIN_N_SCALED, CHAIN_RATIO, scale), grey),
            core.GeometricPrimitive(scaled(em.shape), em.material, core.DiffuseAreaLight((36.0, 36.0, 36.0), 1))]


def node_depths(nodes):
    """Depth of every node of the flattened tree (first child = index + 1, second = offset; the root has depth 0)."""
    depth = np.zeros(len(nodes), np.int32)
    todo = [0]
    while todo:
        i = todo.pop()
        if nodes[i]["nprims"] == 0:
            for c in (i + 1, int(nodes[i]["offset"])):
                depth[c] = depth[i] + 1
                todo.append(c)
    return depth


# ---------------------------------------------------------------------------
# ray constructors
# ---------------------------------------------------------------------------
def _directions(rng, n):
    """Unit directions with every component at least 0.2 in magnitude, both signs of each."""
    d = rng.uniform(0.25, 1.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _pick_targets(rng, nodes, n, solid=False):
    """Half leaves, half interior nodes, uniformly among each (every depth of the tree turns up); solid: only boxes with an
    extent along all three axes (a ray can cross them properly)."""
    ok = np.ones(len(nodes), bool)
    if solid:
        ok = np.all(nodes["bmax"] > nodes["bmin"], axis=1)
    leaves = np.nonzero(ok & (nodes["nprims"] > 0))[0]
    inner = np.nonzero(ok & (nodes["nprims"] == 0))[0]
    t = np.where(rng.random(n) < 0.5, leaves[rng.integers(0, len(leaves), n)], inner[rng.integers(0, len(inner), n)])
    return t


def _reach(rng, bmin, bmax, lo, hi):
    """Distance from the target point to the origin: lo .. hi box diagonals."""
    return np.linalg.norm(bmax - bmin, axis=1) * rng.uniform(lo, hi, len(bmin))


def _spare(n):
    """Candidates drawn for n rays: _finish drops those that meet a triangle at their critical point."""
    return n + n // 4 + 64


def _finish(osc, n, o, d, tmin, tmax, nodes, target, crit=None, agree=True):
    """The first n candidates whose critical parameter `crit` (where the ray touches the target box, or E / X beside maxDistance /
    minDistance) is free of triangles: no triangle of the scene is met within crit (1 +- 2^-10), by exhaustive Triangle.intersect.
    A triangle there is hit at a t that differs from E, X or maxDistance by rounding only -- the box test and the triangle test then
    round differently, and the accelerator legitimately loses a hit that exhaustive testing finds (in the reference too): such rays
    would say nothing about the kernels against the oracle but break the oracle's own check against brute force.
    osc None: no candidate is dropped (the filter against the literal test on one box needs no scene)."""
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    m = len(o)
    tmin = np.broadcast_to(np.asarray(tmin, F64), (m,)).copy()
    tmax = np.broadcast_to(np.asarray(tmax, F64), (m,)).copy()
    keep = np.ones(m, bool)
    if osc is not None:
        from oracle.binding import make_rays
        if crit is not None:
            w = np.abs(crit) * 2.0 ** -10
            keep &= osc.intersect(make_rays(o, d, crit - w, crit + w), brute=True)["prim"] < 0
        # ... and Triangle.intersect (f64) and Triangle.intersectP (f32 temporaries) must agree on whether the ray meets the scene at
        # all, both by exhaustive testing: from an origin 10^30 away the f32 form 'hits' triangles the ray misses by far, in boxes
        # no accelerator visits -- again the reference's arithmetic, and again nothing a box test can be blamed for.  (Not asked of the
        # tiny family, agree False: there the f32 form underflows and never reports a hit, see band_family.)
        rays = make_rays(o, d, tmin, tmax)
        if agree:
            keep &= (osc.intersect(rays, brute=True)["prim"] >= 0) == (osc.intersect(rays, any_hit=True, brute=True)["prim"] >= 0)
    keep = np.nonzero(keep)[0]
    assert len(keep) >= n, (len(keep), n)
    keep = keep[:n]
    o, d, tmin, tmax, target = o[keep], d[keep], tmin[keep], tmax[keep], np.asarray(target)[keep]
    assert np.all(np.isfinite(o)) and np.all(np.isfinite(d)) and np.all(d != 0) and not np.isnan(tmin).any() and not np.isnan(tmax).any()
    sh, sm = slab_f32_sure(o, d, tmin, tmax, nodes["bmin"][target], nodes["bmax"][target])
    return {"o": o, "d": d, "tmin": tmin, "tmax": tmax, "target": target, "ambiguous": ~(sh | sm)}


def edge_rays(osc, nodes, n, seed, zero_free=False):
    """Rays that graze the target box in a point of one of its 12 edges or 8 corners: of the planes through that point the ray
    enters one slab and leaves another, so the entry parameter E and the exit parameter X are equal but for rounding.
    (zero_free: see band_family.)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n, want = _spare(n), n
    t = _pick_targets(rng, nodes, n)
    bmin, bmax = nodes["bmin"][t].astype(F64), nodes["bmax"][t].astype(F64)
    # per axis: 0 = the point lies on the min face, 1 = on the max face, 2 = strictly between (edges: one axis, corners: none)
    side = rng.integers(0, 2, (n, 3))
    along = rng.integers(0, 3, n)
    corner = rng.random(n) < 0.4
    side[~corner, along[~corner]] = 2
    u = rng.uniform(0.1, 0.9, (n, 3))
    p = np.where(side == 0, bmin, np.where(side == 1, bmax, bmin + u * (bmax - bmin)))
    # roles of the planes through the point: enter (True) / leave; at least one of each
    enter = rng.random((n, 3)) < 0.5
    on = side != 2
    n_enter = (enter & on).sum(axis=1)
    same = np.nonzero((n_enter == 0) | (n_enter == on.sum(axis=1)))[0]
    first = np.argmax(on, axis=1)
    enter[same, first[same]] ^= True
    sign = np.where(on, np.where(enter ^ (side == 1), 1.0, -1.0), rng.choice([-1.0, 1.0], (n, 3)))
    d = rng.uniform(0.25, 1.0, (n, 3)) * sign
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (p - d * _reach(rng, bmin, bmax, 0.5, 4.0)[:, None]).astype(F32)
    d = p - o.astype(F64)
    reach = np.linalg.norm(d, axis=1)
    d = (d / reach[:, None]).astype(F32)
    return _finish(osc, want, o, d, reach * 2.0 ** -10 if zero_free else 0.0, np.inf, nodes, t, crit=reach, agree=not zero_free)


def _crossing(rng, nodes, n, behind=None):
    """Rays through a point well inside a solid target box, from 0.5 .. 4 diagonals away (behind: the box lies behind the origin)."""
    t = _pick_targets(rng, nodes, n, solid=True)
    bmin, bmax = nodes["bmin"][t].astype(F64), nodes["bmax"][t].astype(F64)
    q = bmin + rng.uniform(0.2, 0.8, (n, 3)) * (bmax - bmin)
    d = _directions(rng, n)
    reach = _reach(rng, bmin, bmax, 0.5, 4.0)
    if behind is not None:
        reach = np.where(behind, -reach, reach)
    o = (q - d * reach[:, None]).astype(F32)
    d = d.astype(F32)
    _, geom, E, X = slab_f64(o, d, -np.inf, np.inf, nodes["bmin"][t], nodes["bmax"][t])
    assert geom.all() and np.all(E < X)
    return t, o, d, E, X


def _around(v, i):
    """v itself, its two f64 neighbours, and v moved by +-1 and +-2 f32 ulps (variant i mod 7)."""
    ulp = np.spacing(np.abs(v).astype(F32)).astype(F64)
    k = i % 7
    out = np.where(k == 1, np.nextafter(v, np.inf), np.where(k == 2, np.nextafter(v, -np.inf), v))
    step = np.select([k == 3, k == 4, k == 5, k == 6], [1.0, -1.0, 2.0, -2.0], 0.0)
    return out + step * ulp


def tmax_rays(osc, nodes, n, seed, zero_free=False):
    """maxDistance = the target box's entry parameter E (as the literal test computes it) or next to it: `t0 < maxDistance`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = _spare(n)
    t, o, d, E, X = _crossing(rng, nodes, m)
    return _finish(osc, n, o, d, E * 2.0 ** -10 if zero_free else 0.0, _around(E, np.arange(m)), nodes, t, crit=E, agree=not zero_free)


def tmin_rays(osc, nodes, n, seed, zero_free=False):
    """minDistance = the target box's exit parameter X or next to it: `t1 > minDistance`.  Half of the boxes lie behind the origin
    (minDistance < 0), half of those with maxDistance <= 0 (0, or a quarter of X): legal for dr_intersect."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = _spare(n)
    kind = rng.integers(0, 4, m)  # 0, 1: in front; 2: behind; 3: behind and maxDistance <= 0
    t, o, d, E, X = _crossing(rng, nodes, m, behind=kind >= 2)
    tmax = np.where(kind == 3, np.where(rng.random(m) < 0.5, 0.0, 0.25 * X), np.inf)
    if zero_free:
        tmax = np.where(kind >= 2, 0.25 * X, np.inf)
    return _finish(osc, n, o, d, _around(X, np.arange(m)), tmax, nodes, t, crit=X, agree=not zero_free)


def facehit_rays(osc, nodes, tri, mesh, verts, n, seed):
    """Rays aimed at points of the shingle stack's triangles: each lies in a face of the boxes that group the quads of the planes
    next to it (and of its own flat leaf), so the accepted hit's t falls within the band of entries still on the stack -- the
    pop-time re-test and pruneStack.  target = the triangle's own leaf."""
    rng = np.random.Generator(np.random.PCG64(seed))
    prims = np.nonzero(mesh == SHINGLE_MESH)[0]
    pr = prims[rng.integers(0, len(prims), n)]
    leaf_of = np.zeros(len(tri), np.int64)
    for i in np.nonzero(nodes["nprims"] > 0)[0]:
        leaf_of[nodes[i]["offset"]:nodes[i]["offset"] + nodes[i]["nprims"]] = i
    V = verts[tri[pr]].astype(F64)
    b = rng.uniform(0.1, 0.4, (n, 2))
    p = V[:, 0] + b[:, :1] * (V[:, 1] - V[:, 0]) + b[:, 1:] * (V[:, 2] - V[:, 0])
    d = _directions(rng, n)
    o = (p - d * rng.uniform(1.0, 6.0, (n, 1))).astype(F32)
    d = p - o.astype(F64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return _finish(osc, n, o, d, 0.0, np.inf, nodes, leaf_of[pr])


def band_family(name, osc, n, seed=1, clean=True):
    """n rays of family `name` for the oracle scene `osc` of band_prims(SCALES[name]): dict(o, d f32; tmin, tmax f64; target = node
    index; ambiguous = the restated filter leaves the target box to the literal test; tiny / huge also part = 0 edge, 1 tmax,
    2 tmin).  clean False: candidates that meet a triangle at their critical point stay (_finish).

    The tiny family keeps 0 out of [minDistance, maxDistance] (zero_free: minDistance = 2^-10 of the critical parameter for the
    edge and tmax rays, maxDistance = X / 4 < 0 for every box behind the origin).  At 2^-100 the f32 temporaries of
    Triangle.intersectP underflow: cross(o - p1, e1) is 0, so b2 = 0 and t = 0 for EVERY triangle whose b1 lies in [0, 1] -- the
    reference's own arithmetic, which the oracle and the kernels repeat, but with 0 in the ray's interval exhaustive testing then
    finds an 'occluder' wherever the accelerator does not happen to look, and the oracle's check against brute force means nothing."""
    nodes, tri, mesh, _ = osc.bvh()
    verts = osc.verts()
    if not clean:
        osc = None
    if name == "edge":
        return edge_rays(osc, nodes, n, seed)
    if name == "tmax":
        return tmax_rays(osc, nodes, n, seed)
    if name == "tmin":
        return tmin_rays(osc, nodes, n, seed)
    if name == "facehit":
        return facehit_rays(osc, nodes, tri, mesh, verts, n, seed)
    if name in ("tiny", "huge"):
        third = [n - 2 * (n // 3), n // 3, n // 3]
        parts = [f(osc, nodes, m, seed + k, zero_free=name == "tiny") for k, (f, m) in enumerate(zip((edge_rays, tmax_rays, tmin_rays), third))]
        out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        out["part"] = np.repeat(np.arange(3), third)
        return out
    raise ValueError(name)


# ---------------------------------------------------------------------------
# shared by tests/test_band_rays.py and tests/test_gpu_traversal_band.py: built once, never modified
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_scene(scale=1.0):
    import oracle.binding as ob
    return ob.OracleScene(band_prims(scale))


@functools.lru_cache(maxsize=None)
def family(name, n=20000, seed=1):
    """The family's rays as every test uses them, with the oracle's answers: dict of band_family's arrays plus rays (the oracle's
    record array), closest (hit records), occluded (booleans), counters / any_counters (the oracle's, for exactly these rays) and
    far_first (its order study of the any-hit walk)."""
    import oracle.binding as ob
    osc = oracle_scene(SCALES[name])
    r = dict(band_family(name, osc, n, seed))
    r["rays"] = ob.make_rays(r["o"], r["d"], r["tmin"], r["tmax"])
    osc.counters(reset=True)
    r["closest"] = osc.intersect(r["rays"])
    r["counters"] = osc.counters()
    osc.counters(reset=True)
    ob.order_study(True)
    r["occluded"] = osc.intersect(r["rays"], any_hit=True)["prim"] >= 0
    r["far_first"] = ob.order_study(False)
    r["any_counters"] = osc.counters()
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r
