"""Float64 closest-point / signed-distance reference for the mesh SDF kernels (a plain helper module for the tests).

`closest_point_f64` answers, exactly in float64, which face of a triangle mesh is closest to each query point: the
distance, the closest point, the face, and every face whose squared distance lies within the kernels' tie band
`d^2 <= best^2 (1 + 1e-5) + 1e-12` (lg_bvh.h: `closest_grid_triangle`, `closest_point`).  Point-triangle distances use
the Voronoi regions of Ericson, Real-Time Collision Detection, s5.1.5, evaluated on (point, face) pairs in vectorised
chunks.  Faces are pre-filtered by the distance to their axis-aligned box against an upper bound of the answer (the
distance to the nearest vertex of a face that counts): a face whose box is farther than the bound holds no point within
it, so the filter changes nothing.  Zero-area faces (`|cross| <= 1e-10`) are skipped, as the kernels skip them.

`signed_reference` applies the kernels' sign rule on top: among the in-band faces the normal of the face with the
largest `|(p - q) . n|` (positive values weighted by 1.001) decides the sign of `(p - q) . n`, q the closest point."""
from dataclasses import dataclass

import numpy as np

BAND_REL, BAND_ABS = 1e-5, 1e-12       # the kernels' tie band on squared distances
DEGENERATE = 1e-10                     # |cross(b - a, c - a)| at or below this: a zero-area face, skipped


@dataclass
class ClosestF64:
    d: np.ndarray          # (P,) exact unsigned distance to the nearest non-degenerate face
    q: np.ndarray          # (P, 3) closest point
    face: np.ndarray       # (P,) index of the closest face; -1 when d > max_dist
    band_pt: np.ndarray    # (K,) the in-band (point, face) pairs: point index ...
    band_face: np.ndarray  # (K,) ... face index ...
    band_q: np.ndarray     # (K, 3) ... closest point on that face ...
    band_d2: np.ndarray    # (K,) ... and its squared distance

    def band_faces(self, i):
        return self.band_face[self.band_pt == i]


def closest_on_triangles(p, a, b, c):
    """Closest point on triangle (a, b, c) to p, all (K, 3) float64 (Ericson's regions: vertex, edge, interior)."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(1), (ac * ap).sum(1)
    bp = p - b
    d3, d4 = (ab * bp).sum(1), (ac * bp).sum(1)
    cp = p - c
    d5, d6 = (ab * cp).sum(1), (ac * cp).sum(1)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    with np.errstate(divide="ignore", invalid="ignore"):
        den = va + vb + vc
        out = a + (vb / den)[:, None] * ab + (vc / den)[:, None] * ac                 # interior
        e_bc = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        out = np.where(e_bc[:, None], b + w[:, None] * (c - b), out)
        e_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        w = d2 / (d2 - d6)
        out = np.where(e_ac[:, None], a + w[:, None] * ac, out)
        out = np.where(((d6 >= 0) & (d5 <= d6))[:, None], c, out)
        e_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v = d1 / (d1 - d3)
        out = np.where(e_ab[:, None], a + v[:, None] * ab, out)
    # (layered so that the tests Ericson makes first take precedence: a, b, edge ab, c, edge ac, edge bc, interior)
    out = np.where(((d3 >= 0) & (d4 <= d3))[:, None], b, out)
    out = np.where(((d1 <= 0) & (d2 <= 0))[:, None], a, out)
    return out


def _faces(vertices, triangles):
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    tri = v[t]                                                                         # (T, 3, 3)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nl = np.linalg.norm(n, axis=1)
    keep = np.nonzero(nl > DEGENERATE)[0]
    return tri, n, nl, keep


def closest_point_f64(vertices, triangles, points, max_dist, chunk=256):
    tri, _, _, keep = _faces(vertices, triangles)
    ft = tri[keep]
    lo, hi = ft.min(axis=1), ft.max(axis=1)                                            # (F, 3) face boxes
    verts = np.unique(ft.reshape(-1, 3), axis=0)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    P = len(p)
    d = np.empty(P); q = np.empty((P, 3)); face = np.empty(P, np.int64)
    bp, bf, bq, bd = [], [], [], []
    for s in range(0, P, chunk):
        pc = p[s:s + chunk]
        ub2 = ((pc[:, None, :] - verts[None]) ** 2).sum(2).min(1)                     # nearest vertex of a counted face: an upper bound
        box2 = np.zeros((len(pc), len(ft)))
        for k in range(3):
            g = np.maximum(np.maximum(lo[None, :, k] - pc[:, None, k], 0.0), pc[:, None, k] - hi[None, :, k])
            box2 += g * g
        lim = ub2 * (1 + 2 * BAND_REL) + 2 * BAND_ABS                                 # the band of any face that can be the closest
        ip, jf = np.nonzero(box2 <= lim[:, None])
        qq = closest_on_triangles(pc[ip], ft[jf, 0], ft[jf, 1], ft[jf, 2])
        d2 = ((pc[ip] - qq) ** 2).sum(1)
        best = np.full(len(pc), np.inf)
        np.minimum.at(best, ip, d2)
        arg = np.full(len(pc), -1)
        at = np.nonzero(d2 == best[ip])[0]
        arg[ip[at[::-1]]] = at[::-1]                                                   # (the first pair that reaches the minimum)
        d[s:s + len(pc)] = np.sqrt(best)
        q[s:s + len(pc)] = qq[arg]
        face[s:s + len(pc)] = keep[jf[arg]]
        inb = d2 <= best[ip] * (1 + BAND_REL) + BAND_ABS
        bp.append(ip[inb] + s); bf.append(keep[jf[inb]]); bq.append(qq[inb]); bd.append(d2[inb])
    face = np.where(d > max_dist, -1, face)
    return ClosestF64(d, q, face, np.concatenate(bp), np.concatenate(bf), np.concatenate(bq).reshape(-1, 3), np.concatenate(bd))


@dataclass
class SignedF64:
    sdf: np.ndarray        # (P,) signed distance (max_dist where nothing is within max_dist)
    sign: np.ndarray       # (P,) +1 / -1
    normal: np.ndarray     # (P, 3) unit normal of the deciding face
    sure: np.ndarray       # (P,) the sign decision is unambiguous: every in-band face agrees and |d| > 1e-4
    unique: np.ndarray     # (P,) every in-band face has the same closest point (to 1e-7): the gradient is well defined
    ref: ClosestF64


def signed_reference(vertices, triangles, points, max_dist, chunk=256):
    r = closest_point_f64(vertices, triangles, points, max_dist, chunk)
    tri, n, nl, _ = _faces(vertices, triangles)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    P = len(p)
    nh = n[r.band_face] / nl[r.band_face, None]
    sd = ((p[r.band_pt] - r.band_q) * nh).sum(1)                                        # each face's own plane distance
    key = np.abs(sd) * np.where(sd > 0, 1.001, 1.0)
    top = np.full(P, -np.inf)
    np.maximum.at(top, r.band_pt, key)
    win = np.nonzero(key == top[r.band_pt])[0]
    pick = np.full(P, -1)
    pick[r.band_pt[win[::-1]]] = win[::-1]
    normal = nh[pick]
    diff = p - r.q
    sign = np.where((diff * normal).sum(1) < 0, -1.0, 1.0)
    # a kernel takes its closest point from one in-band face and its normal from another, which one is down to fp32 rounding: the
    # decision is unambiguous when every (point of face f, normal of face g) pair of in-band faces gives the same sign, clear of rounding
    clear = (np.abs(sd) > 1e-6) & (np.sign(sd) == sign[r.band_pt])
    agree = np.ones(P, bool)
    np.logical_and.at(agree, r.band_pt, clear)
    cnt = np.bincount(r.band_pt, minlength=P)
    for i in np.nonzero(agree & (cnt > 1))[0]:
        at = np.nonzero(r.band_pt == i)[0]
        s = ((p[i] - r.band_q[at])[:, None, :] * nh[at][None, :, :]).sum(2)            # [f, g]
        agree[i] = bool(((np.abs(s) > 1e-6) & (np.sign(s) == sign[i])).all())
    gap = np.linalg.norm(r.band_q - r.q[r.band_pt], axis=1)
    unique = np.ones(P, bool)
    np.logical_and.at(unique, r.band_pt, gap <= 1e-7)
    far = r.d > max_dist
    sdf = np.where(far, max_dist, sign * r.d)
    return SignedF64(sdf, sign, normal, agree & (r.d > 1e-4) & ~far, unique, r)
