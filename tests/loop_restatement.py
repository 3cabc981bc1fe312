"""DESIGN.md 2.10 (Shape "loopsubdiv") restated in plain Python: LoopSubdivision's constructor and refine()
(shapes/loop_subdivision.dart:23-516) in the reference's own pointer style -- objects for _SDVertex / _SDFace / _SDEdge, dicts of dicts for
the edge maps -- with Point / Vector arithmetic as core/vector.dart:27-74 and core/point.dart:35-45 have it: components stored as f32
(numpy.float32 after every operator), every operator computed in f64.  Written apart from dartray_amd.core and from the C++ / HIP builders
(flat arrays, sorted edge list, prefix sums): it shares no code with them.  Cited by file.dart:line of the reference.

Math.cos / Math.sin are Python's, i.e. the C library's: the stated departure of DESIGN.md 2.10.

Only meshes the reference itself survives go in here: it crashes or loops on the inputs the builders refuse.
"""
import math

import numpy as np


def _f32(x):
    return float(np.float32(x))


class Vec:
    """Vector / Point / Normal: a Float32List of 3 (vector.dart:27-34); an operator makes a new one from f64 results."""
    __slots__ = ("x", "y", "z")

    def __init__(self, x=0.0, y=0.0, z=0.0):
        self.x, self.y, self.z = _f32(x), _f32(y), _f32(z)

    def __add__(self, o):                                           # vector.dart:57-60, point.dart:41-42
        return Vec(self.x + o.x, self.y + o.y, self.z + o.z)

    def __sub__(self, o):                                           # vector.dart:62-65, point.dart:44-45
        return Vec(self.x - o.x, self.y - o.y, self.z - o.z)

    def __mul__(self, f):                                           # vector.dart:67-68, point.dart:35-36
        return Vec(self.x * f, self.y * f, self.z * f)

    def __neg__(self):                                              # vector.dart:73-74
        return Vec(-self.x, -self.y, -self.z)


def Cross(v1, v2):                                                  # vector.dart:158-168
    return Vec((v1.y * v2.z) - (v1.z * v2.y), (v1.z * v2.x) - (v1.x * v2.z), (v1.x * v2.y) - (v1.y * v2.x))


class _SDVertex:                                                    # :404-460
    def __init__(self, P):
        self.P = P
        self.startFace = None
        self.child = None
        self.regular = False
        self.boundary = False

    def valence(self):                                              # :409-430
        f = self.startFace
        if not self.boundary:
            nf = 1
            while True:
                f = f.nextFace(self)
                if f is self.startFace:
                    break
                nf += 1
            return nf
        nf = 1
        while True:
            f = f.nextFace(self)
            if f is None:
                break
            nf += 1
        f = self.startFace
        while True:
            f = f.prevFace(self)
            if f is None:
                break
            nf += 1
        return nf + 1

    def oneRing(self):                                              # :432-453 (returns the list it fills)
        p = []
        if not self.boundary:
            face = self.startFace
            while True:
                p.append(face.nextVert(self).P)
                face = face.nextFace(self)
                if face is self.startFace:
                    break
        else:
            face = self.startFace
            while True:
                f2 = face.nextFace(self)
                if f2 is None:
                    break
                face = f2
            p.append(face.nextVert(self).P)
            while True:
                p.append(face.prevVert(self).P)
                face = face.prevFace(self)
                if face is None:
                    break
        return p


class _SDFace:                                                      # :462-502
    def __init__(self):
        self.v = [None, None, None]
        self.f = [None, None, None]
        self.children = [None, None, None, None]

    def vnum(self, vert):
        for i in range(3):
            if self.v[i] is vert:
                return i
        raise AssertionError("Basic logic error in SDFace::vnum()")

    def nextFace(self, vert):
        return self.f[self.vnum(vert)]

    def prevFace(self, vert):
        return self.f[(self.vnum(vert) + 2) % 3]

    def nextVert(self, vert):
        return self.v[(self.vnum(vert) + 1) % 3]

    def prevVert(self, vert):
        return self.v[(self.vnum(vert) + 2) % 3]

    def otherVert(self, v0, v1):
        for i in range(3):
            if self.v[i] is not v0 and self.v[i] is not v1:
                return self.v[i]
        raise AssertionError("Basic logic error in SDVertex::otherVert()")


class _SDEdge:                                                      # :504-514
    def __init__(self, v0, v1):
        self.v = [v0, v1]
        self.f = [None, None]
        self.f0edgeNum = -1


class _SDEdgeMap:                                                   # :379-402 (objects hash by identity, as in Dart)
    def __init__(self):
        self._edgeMap = {}

    def getEdge(self, a, b):
        if a in self._edgeMap and b in self._edgeMap[a]:
            return self._edgeMap[a][b]
        if b in self._edgeMap and a in self._edgeMap[b]:
            return self._edgeMap[b][a]
        return None

    def setEdge(self, a, b, v):
        self._edgeMap.setdefault(a, {})[b] = v


def Beta(valence):                                                  # :326-331
    if valence == 3:
        return 3.0 / 16.0
    return 3.0 / (8.0 * valence)


def Gamma(valence):                                                 # :356-358
    return 1.0 / (valence + 3.0 / (8.0 * Beta(valence)))


def WeightOneRing(vert, beta):                                      # :333-343
    valence = vert.valence()
    Pring = vert.oneRing()
    P = vert.P * (1.0 - valence * beta)
    for i in range(valence):
        P = P + Pring[i] * beta
    return P


def WeightBoundary(vert, beta):                                     # :345-354
    valence = vert.valence()
    Pring = vert.oneRing()
    P = vert.P * (1.0 - 2.0 * beta)
    P = P + Pring[0] * beta
    P = P + Pring[valence - 1] * beta
    return P


class LoopSubdivision:
    def __init__(self, vertexIndices, P, nLevels):                  # :24-93
        P = np.asarray(P, np.float32).reshape(-1, 3)
        vertexIndices = [int(i) for i in np.asarray(vertexIndices).reshape(-1)]
        nfaces = len(vertexIndices) // 3
        self.nLevels = nLevels
        self.vertices = [_SDVertex(Vec(*[float(c) for c in p])) for p in P]
        self.faces = []
        j = 0
        for _ in range(nfaces):
            f = _SDFace()
            self.faces.append(f)
            for k in range(3):
                v = self.vertices[vertexIndices[j]]
                j += 1
                f.v[k] = v
                v.startFace = f
        edges = _SDEdgeMap()
        for f in self.faces:
            for ei in range(3):
                v0, v1 = f.v[ei], f.v[(ei + 1) % 3]
                edge = edges.getEdge(v0, v1)
                if edge is None:
                    edge = _SDEdge(v0, v1)
                    edge.f[0] = f
                    edge.f0edgeNum = ei
                    edges.setEdge(v0, v1, edge)
                else:
                    edge.f[0].f[edge.f0edgeNum] = f
                    f.f[ei] = edge.f[0]
        for v in self.vertices:
            f = v.startFace
            while True:
                f = f.nextFace(v)
                if f is None or f is v.startFace:
                    break
            v.boundary = f is None
            val = v.valence()
            if not v.boundary and val == 6:
                v.regular = True
            elif v.boundary and val == 4:
                v.regular = True
            else:
                v.regular = False

    def refine(self):                                               # :99-308 -> (P, N, indices) of the TriangleMesh it creates
        f, v = self.faces, self.vertices
        for _ in range(self.nLevels):
            newFaces, newVertices = [], []
            for vert in v:                                          # :109-114
                vert.child = _SDVertex(None)
                vert.child.regular = vert.regular
                vert.child.boundary = vert.boundary
                newVertices.append(vert.child)
            for face in f:                                          # :116-121
                for k in range(4):
                    face.children[k] = _SDFace()
                    newFaces.append(face.children[k])
            for vert in v:                                          # :126-138
                if not vert.boundary:
                    if vert.regular:
                        vert.child.P = WeightOneRing(vert, 1.0 / 16.0)
                    else:
                        vert.child.P = WeightOneRing(vert, Beta(vert.valence()))
                else:
                    vert.child.P = WeightBoundary(vert, 1.0 / 8.0)
            edgeVerts = _SDEdgeMap()                                # :141-172
            for face in f:
                for k in range(3):
                    fv1, fv2 = face.v[k], face.v[(k + 1) % 3]
                    vert = edgeVerts.getEdge(fv1, fv2)
                    if vert is None:
                        vert = _SDVertex(None)
                        newVertices.append(vert)
                        vert.regular = True
                        vert.boundary = face.f[k] is None
                        vert.startFace = face.children[3]
                        if vert.boundary:
                            vert.P = fv1.P * 0.5 + fv2.P * 0.5
                        else:
                            vert.P = fv1.P * (3.0 / 8.0) + fv2.P * (3.0 / 8.0)
                            vert.P = vert.P + face.otherVert(fv1, fv2).P * (1.0 / 8.0)
                            vert.P = vert.P + face.f[k].otherVert(fv1, fv2).P * (1.0 / 8.0)
                        edgeVerts.setEdge(fv1, fv2, vert)
            for vert in v:                                          # :177-181
                vertNum = vert.startFace.vnum(vert)
                vert.child.startFace = vert.startFace.children[vertNum]
            for face in f:                                          # :184-202
                for k in range(3):
                    face.children[3].f[k] = face.children[(k + 1) % 3]
                    face.children[k].f[(k + 1) % 3] = face.children[3]
                    f2 = face.f[k]
                    face.children[k].f[k] = f2.children[f2.vnum(face.v[k])] if f2 is not None else None
                    f2 = face.f[(k + 2) % 3]
                    face.children[k].f[(k + 2) % 3] = f2.children[f2.vnum(face.v[k])] if f2 is not None else None
            for face in f:                                          # :205-220
                for k in range(3):
                    face.children[k].v[k] = face.v[k].child
                    vert = edgeVerts.getEdge(face.v[k], face.v[(k + 1) % 3])
                    face.children[k].v[(k + 1) % 3] = vert
                    face.children[(k + 1) % 3].v[k] = vert
                    face.children[3].v[k] = vert
            f, v = newFaces, newVertices

        Plimit = []                                                 # :228-239
        for vert in v:
            if vert.boundary:
                Plimit.append(WeightBoundary(vert, 1.0 / 5.0))
            else:
                Plimit.append(WeightOneRing(vert, Gamma(vert.valence())))
        for i, vert in enumerate(v):
            vert.P = Plimit[i]

        Ns = []                                                     # :242-283
        for vert in v:
            S, T = Vec(), Vec()
            valence = vert.valence()
            Pring = vert.oneRing()
            if not vert.boundary:
                for k in range(valence):
                    S = S + Pring[k] * (math.cos(2.0 * math.pi * k / valence))
                    T = T + Pring[k] * (math.sin(2.0 * math.pi * k / valence))
            else:
                S = Pring[valence - 1] - Pring[0]
                if valence == 2:
                    T = Pring[0] + Pring[1] - vert.P * 2.0
                elif valence == 3:
                    T = Pring[1] - vert.P
                elif valence == 4:
                    T = Pring[0] * -1.0 + Pring[1] * 2.0 + Pring[2] * 2.0 + Pring[3] * -1.0 + vert.P * -2.0
                else:
                    theta = math.pi / (valence - 1)
                    T = (Pring[0] + Pring[valence - 1]) * math.sin(theta)
                    for k in range(1, valence - 1):
                        wt = (2 * math.cos(theta) - 2) * math.sin(k * theta)
                        T = T + Pring[k] * wt
                    T = -T
            Ns.append(Cross(S, T))

        usedVerts = {vert: i for i, vert in enumerate(v)}           # :286-299
        verts = np.array([[usedVerts[face.v[j]] for j in range(3)] for face in f], dtype=np.uint32)
        P = np.array([[p.x, p.y, p.z] for p in Plimit], dtype=np.float32)
        N = np.array([[n.x, n.y, n.z] for n in Ns], dtype=np.float32)
        return P, N, verts


def refine(indices, P, nlevels):
    return LoopSubdivision(indices, P, nlevels).refine()
