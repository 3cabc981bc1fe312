"""Control meshes of the Loop subdivision tests (tests/test_loop_subdivision.py, tests/test_gpu_subdiv.py): name -> (indices [nf,3] uint32,
P [nv,3] float32).  Each one is there for the branch its valences take; none is planar, so that no normal is trivially
parallel to an axis."""
import math

import numpy as np


def _mesh(faces, P):
    return np.asarray(faces, np.uint32).reshape(-1, 3), np.asarray(P, np.float64).astype(np.float32).reshape(-1, 3)


def bipyramid(n, height=1.0):
    """Ring of n vertices, apices n (top) and n + 1 (bottom): apex valence n, ring valence 4."""
    P = [(math.cos(2 * math.pi * i / n), math.sin(2 * math.pi * i / n), 0.1 * math.sin(3.0 * i)) for i in range(n)]
    P += [(0.0, 0.0, height), (0.05, 0.0, -0.8 * height)]
    faces = []
    for i in range(n):
        j = (i + 1) % n
        faces += [(i, j, n), (j, i, n + 1)]
    return _mesh(faces, P)


def grid(n):
    """n x n vertices, every cell cut along the same diagonal: interior valence 6, boundary valence 4, corners 2 and 3."""
    P = [(x / (n - 1), y / (n - 1), 0.3 * math.sin(1.7 * x + y)) for y in range(n) for x in range(n)]
    faces = []
    for y in range(n - 1):
        for x in range(n - 1):
            a, b, c, d = x + y * n, x + 1 + y * n, x + 1 + (y + 1) * n, x + (y + 1) * n
            faces += [(a, b, c), (a, c, d)]
    return _mesh(faces, P)


def fan(n):
    """n triangles about boundary vertex 0: its valence is n + 1."""
    P = [(0.0, 0.0, 0.2)] + [(math.cos(math.pi * i / n), math.sin(math.pi * i / n), 0.15 * math.cos(2.0 * i)) for i in range(n + 1)]
    return _mesh([(0, i, i + 1) for i in range(1, n + 1)], P)


def tetrahedron():
    return _mesh([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], [(1, 1, 1), (1, -1, -1.1), (-1, 1.2, -1), (-0.9, -1, 1)])


def icosahedron():
    t = (1.0 + math.sqrt(5.0)) / 2.0
    P = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    return _mesh(faces, P)


MESHES = {
    "tetrahedron": tetrahedron(),                                             # interior valence 3: Beta(3)
    "octahedron": bipyramid(4),                                               # valence 4
    "icosahedron": icosahedron(),                                             # valence 5
    "bipyramid9": bipyramid(9),                                               # apex valence 9, ring valence 4
    "triangle": _mesh([(0, 1, 2)], [(0, 0, 0), (1, 0, 0.1), (0.2, 1, -0.1)]),  # boundary valence 2
    "quad": _mesh([(0, 1, 2), (0, 2, 3)], [(0, 0, 0), (1, 0, 0.2), (1.1, 1, 0), (0, 0.9, 0.3)]),  # corners of valence 2 and 3
    "grid3": grid(3),                                                         # boundary valence 4 (regular), interior valence 6
    "fan4": fan(4),                                                           # boundary valence 5: the general boundary branch
    "fan6": fan(6),                                                           # boundary valence 7
}
LEVELS = (0, 1, 2, 3)


def fuzz_case(seed):
    """One of MESHES with its face order permuted, every face's indices rotated and its positions jittered: (name, indices, P)."""
    rng = np.random.RandomState(1000 + seed)
    name = sorted(MESHES)[rng.randint(len(MESHES))]
    idx, P = MESHES[name]
    idx = idx[rng.permutation(len(idx))]
    idx = np.stack([np.roll(f, int(rng.randint(3))) for f in idx]).astype(np.uint32)
    P = (P.astype(np.float64) + rng.uniform(-0.05, 0.05, P.shape)).astype(np.float32)
    return name, np.ascontiguousarray(idx), np.ascontiguousarray(P)


def euler_counts(idx, nlevels):
    """Faces and vertices of the refined mesh: a level keeps the vertices, adds one per edge, and V - E + F stays what it is."""
    nf, nv = len(idx), int(idx.max()) + 1
    ne = len({tuple(sorted((int(f[k]), int(f[(k + 1) % 3])))) for f in idx for k in range(3)})
    for _ in range(nlevels):
        nv, ne, nf = nv + ne, 2 * ne + 3 * nf, 4 * nf
    return nf, nv


def _refusal(faces, nverts, nlevels, message):
    rng = np.random.RandomState(7)
    return np.asarray(faces, np.uint32).reshape(-1, 3), rng.uniform(-1, 1, (nverts, 3)).astype(np.float32), nlevels, message


# name -> (indices, P, nlevels, what dr_last_error says): every input the reference crashes or loops on
REFUSALS = {
    "unused_vertex": _refusal([(0, 1, 2)], 4, 1, "a vertex is named by no face"),
    "index_out_of_range": _refusal([(0, 1, 5)], 3, 1, "a vertex index is out of range"),
    "repeated_vertex": _refusal([(0, 1, 2), (2, 1, 1)], 3, 1, "a face repeats a vertex"),
    "edge_of_three_faces": _refusal([(0, 1, 2), (1, 0, 3), (0, 1, 4)], 5, 1, "an edge is shared by more than two faces"),
    "same_direction": _refusal([(0, 1, 2), (0, 1, 3)], 4, 1, "two faces traverse a shared edge in the same direction"),
    "bow_tie": _refusal([(0, 1, 2), (0, 3, 4)], 5, 1, "the faces of a vertex do not form one fan"),
    "negative_nlevels": _refusal([(0, 1, 2)], 3, -1, "nlevels is negative"),
    "too_many_faces": MESHES["icosahedron"] + (14, "2\\^31 or more faces or vertices"),   # 20 * 4^14 faces
    "too_many_faces_open": MESHES["triangle"] + (16, "2\\^31 or more faces or vertices"),  # 4^16 faces (vertices never outnumber 3 x faces)
}
