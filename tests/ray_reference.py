"""Float64 bounds for the ray kernels (a plain helper module for the tests): ray casts, the ray-caster sensor, the depth camera.

The kernels' `ray_triangle` (csrc/lg_bvh.h) is Moller-Trumbore in fp32 with a barycentric band B = RAY_EDGE_EPS.  Nothing here repeats
that arithmetic: `ray_bounds` evaluates u, v, t and det of every (ray, face) pair in float64 on the same fp32 inputs, and next to each a
bound on what ANY fp32 evaluation of the same formulas can be off by.  From those it forms two sets per ray:

  inner   pairs every correct fp32 evaluation MUST accept:  -B + eu <= u <= T1 - eu,  v >= -B + ev,  u + v <= T1 - euv,  et <= t <= max_dist - et
  outer   pairs it MAY accept: the same tests with the bounds on the other side

(T1 = fl32(1 + B), the kernels' own constant).  `t_in = min over inner (t + et)`, `t_out = min over outer (t - et)`, inf when empty.  A correct
walk over ANY acceleration structure answers t_out <= t_kernel <= t_in on every ray, a miss counting as inf; no ray is exempt.  A ray is
`tight` when both are inf, or t_in - t_out <= TIGHT * et: there hit / miss is decided and t is pinned to rounding.

The rounding bound (u = 2^-24, fp32 round to nearest, no contraction needed: a fused product only drops a rounding).  Per pair, with
e1 = b - a, e2 = c - a, s = o - a (one rounding per component each), p = d x e2, q = s x e1 and |x| the componentwise absolute value:

  p_i  = d_j e2_k - d_k e2_j          3 roundings (e2, product, difference) relative to P_i = |d_j||e2_k| + |d_k||e2_j|
  det  = (e1x px + e1y py) + e1z pz   e1 1 + p 3 + product 1 + two sums 2 = 7 relative to Sdet = sum |e1_i| P_i
  u det = s . p                        7 relative to Su = sum |s_i| P_i
  q_i                                  4 roundings (s, e1, product, difference) relative to Q_i = |s_j||e1_k| + |s_k||e1_j|
  v det = d . q                        q 4 + product 1 + sums 2 = 7 relative to Sv = sum |d_i| Q_i
  t det = e2 . q                       e2 1 + q 4 + product 1 + sums 2 = 8 relative to St = sum |e2_i| Q_i

so no numerator is more than 8 roundings deep and K = 9 covers gamma_8 = 8u / (1 - 8u) with room: E(x) = K u S(x).  The quotient
x = fl(X * fl(1 / det)) adds 2 roundings and the error of det: with rel = E(det) / |det| < 1,

  ex = (E(X) / |det| + |x| (rel + 3u)) / (1 - rel)

-- the issue's `K u (sum of absolute products) / |det|  +  |x| (the same for det)`, with the reciprocal's non-linearity kept.  The sum u + v
adds one rounding: euv = eu + ev + u (|u + v| + eu + ev).  K is derived, not fitted: tests/test_ray_reference.py confirms it against the CPU
oracle's fp32 scan only, never against a kernel.

A pair is `resolved` when rel <= 1/2, |det| - E(det) >= 1e-20 (the kernels' determinant test cannot drop it), and eu, ev <= 1e-3,
et |d| <= 1e-3 m.  A pair that is not (a ray edge-on to the face, or so far away that rounding swamps the band) is never inner, and is outer
from the parameter at which the ray enters the face's box -- provided its numerators allow |u|, |v| <= T1 at all: |X| - E(X) <= T1 (|det| + E(det)),
which for an edge-on ray says that it runs within rounding of the face's plane (a heightfield folded by the slope correction has hundreds of
vertical faces whose box is a whole cell; without this every vertical ray over such a cell would be left undecided).  Zero-area faces (float64 |e1 x e2| <= 1e-10, `mesh_reference.DEGENERATE`) are
skipped.  Box prefilter: a face whose box, padded by BOX_PAD of its diagonal + 1e-6, the segment [-tpad, max_dist + tpad] misses is in
neither set -- a resolved outer pair has its float64 hit point within (B + 1e-3) (|e1| + |e2|) of the face and its t within 1e-3 m of the
segment, which the padding covers.

Rays known only to a bound (the sensors form o, d in fp32 from a pose): u det, v det, t det and det are bilinear in (o, d), so a ray within
|do| <= oe, |dd| <= de of the float64 one moves them by at most

  det: de |e1 x e2|     u det: oe |p| + de |e2 x s| + oe de |e2|     v det: oe |e1 x d| + de |q| + oe de |e1|     t det: oe |e1 x e2|

which `ray_bounds(..., o_err=, d_err=)` adds to E(.).  Where those bounds come from: `quat_apply_err` -- b + w t + xyz x t with
t = 2 xyz x b, as a running error: dt = u (A + |t|) (the two products, their difference; A = 2 |xyz| x |b|), dc = |xyz| x dt + u (|xyz| x |t| + |c|)
for c = xyz x t, and for the result |w| dt + u |w t| + u |b + w t| + dc + u |result|; yaw-only adds the 3 roundings of q / sqrt(z^2 + w^2), which
move the bilinear part by 2 * 3u (|w| A + |xyz| x A); the sum with the base position adds u |o|.

`raycaster_reference` and `depth_reference` carry the bounds on t through the sensors' own arithmetic (hit point, distance from the BASE,
0 on a miss; depth = -t |d| + noise, clip, Keys bicubic a = -0.75 with align_corners = False and border clamp, normalisation, FIFO) as
intervals, every further fp32 step with a stated term (see the functions)."""
from dataclasses import dataclass

import numpy as np

from tests.mesh_reference import DEGENERATE

U = 2.0 ** -24
K = 9
B = float(np.float32(1e-5))                                   # RAY_EDGE_EPS as the kernels hold it
T1 = float(np.float32(1.0) + np.float32(1e-5))                # fl32(1.f + RAY_EDGE_EPS)
DET_MIN = float(np.float32(1e-20))
TIGHT = 4.0
BOX_PAD = 4e-3
LOOSE = 1e-3                                                  # eu, ev, et |d| above this: the pair is treated like an unresolved one


def _abscross(x, y):
    return np.stack([x[:, 1] * y[:, 2] + x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] + x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] + x[:, 1] * y[:, 0]], axis=1)


def _dot(x, y):
    return (x * y).sum(1)


def _seg_min(idx, val, n):
    """min of val per idx (inf where none) and the position of the pair that reaches it (-1 where none)"""
    best = np.full(n, np.inf)
    pos = np.full(n, -1, np.int64)
    if len(idx):
        order = np.lexsort((val, idx))
        first = np.ones(len(order), bool)
        first[1:] = idx[order][1:] != idx[order][:-1]
        at = order[first]
        best[idx[at]] = val[at]
        pos[idx[at]] = at
    return best, pos


@dataclass
class RayBounds:
    t_in: np.ndarray        # (R,) every correct walk answers <= this (inf: it may miss)
    t_out: np.ndarray       # (R,) ... and >= this (inf: it must miss)
    face_in: np.ndarray     # (R,) the faces that decide them, -1 where none
    face_out: np.ndarray
    et: np.ndarray          # (R,) rounding of t on the deciding face (inner, else outer, else 0)
    tight: np.ndarray       # (R,) hit / miss decided and t pinned to TIGHT * et

    @property
    def must_hit(self):
        return np.isfinite(self.t_in)

    @property
    def must_miss(self):
        return ~np.isfinite(self.t_out)


def faces_of(vertices, triangles):
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    tri = v[np.asarray(triangles, np.int64).reshape(-1, 3)]
    keep = np.nonzero(np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) > DEGENERATE)[0]
    return tri, keep


def ray_bounds(vertices, triangles, origins, dirs, max_dist, o_err=None, d_err=None, pair_budget=2_000_000):
    tri, keep = faces_of(vertices, triangles)
    ft = tri[keep]
    lo, hi = ft.min(axis=1), ft.max(axis=1)
    pad = BOX_PAD * np.linalg.norm(hi - lo, axis=1, keepdims=True) + 1e-6
    lo, hi = lo - pad, hi + pad
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    R = len(o)
    oe = np.zeros(R) if o_err is None else np.broadcast_to(np.asarray(o_err, np.float64), (R,)).copy()
    de = np.zeros(R) if d_err is None else np.broadcast_to(np.asarray(d_err, np.float64), (R,)).copy()
    md = float(np.float32(max_dist))
    out = RayBounds(np.full(R, np.inf), np.full(R, np.inf), np.full(R, -1, np.int64), np.full(R, -1, np.int64), np.zeros(R), np.zeros(R, bool))
    chunk = max(1, pair_budget // max(1, len(ft)))
    for s0 in range(0, R, chunk):
        oc, dc = o[s0:s0 + chunk], d[s0:s0 + chunk]
        n = len(oc)
        dn = np.linalg.norm(dc, axis=1)
        live = dn > 0
        with np.errstate(all="ignore"):
            tpad = np.where(live, (LOOSE + oe[s0:s0 + n]) / np.where(live, dn, 1.0), 0.0)
            ta = np.broadcast_to((-tpad)[:, None], (n, len(ft))).copy()
            tb = np.broadcast_to((md + tpad)[:, None], (n, len(ft))).copy()
            for k in range(3):
                ok, dk = oc[:, k, None], dc[:, k, None]
                mv = dk != 0
                inv = 1.0 / np.where(mv, dk, 1.0)
                t1, t2 = (lo[None, :, k] - ok) * inv, (hi[None, :, k] - ok) * inv
                inside = (ok >= lo[None, :, k]) & (ok <= hi[None, :, k])
                ta = np.maximum(ta, np.where(mv, np.minimum(t1, t2), np.where(inside, -np.inf, np.inf)))
                tb = np.minimum(tb, np.where(mv, np.maximum(t1, t2), np.where(inside, np.inf, -np.inf)))
        ip, jf = np.nonzero((ta <= tb) & live[:, None])
        t_enter = np.maximum(ta[ip, jf], 0.0)
        a, b, c = ft[jf, 0], ft[jf, 1], ft[jf, 2]
        po, pd = oc[ip], dc[ip]
        poe, pde = oe[s0 + ip], de[s0 + ip]
        e1, e2, sv = b - a, c - a, po - a
        p, P = np.cross(pd, e2), _abscross(np.abs(pd), np.abs(e2))
        q, Q = np.cross(sv, e1), _abscross(np.abs(sv), np.abs(e1))
        nrm = np.linalg.norm(np.cross(e1, e2), axis=1)
        det = _dot(e1, p)
        Edet = K * U * _dot(np.abs(e1), P) + pde * nrm
        Eun = K * U * _dot(np.abs(sv), P) + poe * np.linalg.norm(p, axis=1) + pde * np.linalg.norm(np.cross(e2, sv), axis=1) + poe * pde * np.linalg.norm(e2, axis=1)
        Evn = K * U * _dot(np.abs(pd), Q) + poe * np.linalg.norm(np.cross(e1, pd), axis=1) + pde * np.linalg.norm(q, axis=1) + poe * pde * np.linalg.norm(e1, axis=1)
        Etn = K * U * _dot(np.abs(e2), Q) + poe * nrm
        with np.errstate(all="ignore"):
            ad = np.abs(det)
            rel = np.where(ad > 0, Edet / ad, np.inf)
            ok = rel <= 0.5
            sd = np.where(ok, det, 1.0)
            g = 1.0 / (1.0 - np.where(ok, rel, 0.0))
            un, vn = _dot(sv, p), _dot(pd, q)
            uu, vv, tt = un / sd, vn / sd, _dot(e2, q) / sd
            eu = (Eun / np.abs(sd) + np.abs(uu) * (rel + 3 * U)) * g
            ev = (Evn / np.abs(sd) + np.abs(vv) * (rel + 3 * U)) * g
            et = (Etn / np.abs(sd) + np.abs(tt) * (rel + 3 * U)) * g
            euv = eu + ev + U * (np.abs(uu + vv) + eu + ev)
            res = ok & (ad - Edet >= DET_MIN) & (eu <= LOOSE) & (ev <= LOOSE) & (et * dn[ip] <= LOOSE)
            inner = res & (uu >= -B + eu) & (uu <= T1 - eu) & (vv >= -B + ev) & (uu + vv <= T1 - euv) & (tt >= et) & (tt <= md - et)
            outer = res & (uu >= -B - eu) & (uu <= T1 + eu) & (vv >= -B - ev) & (uu + vv <= T1 + euv) & (tt >= -et) & (tt <= md + et)
        k_in = np.nonzero(inner)[0]
        tin, pin = _seg_min(ip[k_in], (tt + et)[k_in], n)
        # an unresolved pair can still only be accepted if |u| <= T1 and |v| <= T1 came out of ITS numerators and determinant: |X| - E(X) <= T1 (|det| + E(det))
        # (for an edge-on ray: the ray lies within rounding of the face's plane, not merely in its box)
        cap = 1.0001 * T1 * (ad + Edet)
        maybe = ~res & (np.abs(un) - Eun <= cap) & (np.abs(vn) - Evn <= cap)
        k_out = np.nonzero(outer | maybe)[0]
        v_out = np.where(res, np.maximum(tt - et, 0.0), t_enter)[k_out]
        v_out = np.where(v_out <= md, v_out, np.inf)
        tout, pout = _seg_min(ip[k_out], v_out, n)
        pout = np.where(np.isfinite(tout), pout, -1)
        sl = slice(s0, s0 + n)
        out.t_in[sl], out.t_out[sl] = tin, tout
        out.face_in[sl] = np.where(pin >= 0, keep[jf[k_in[np.maximum(pin, 0)]]] if len(k_in) else -1, -1)
        out.face_out[sl] = np.where(pout >= 0, keep[jf[k_out[np.maximum(pout, 0)]]] if len(k_out) else -1, -1)
        e_in = et[k_in[np.maximum(pin, 0)]] if len(k_in) else np.zeros(n)
        e_out = np.where(res, et, 0.0)[k_out[np.maximum(pout, 0)]] if len(k_out) else np.zeros(n)
        out.et[sl] = np.where(pin >= 0, e_in, np.where(pout >= 0, e_out, 0.0))
    out.t_out = np.minimum(out.t_out, out.t_in)
    both_inf = ~np.isfinite(out.t_in) & ~np.isfinite(out.t_out)
    with np.errstate(invalid="ignore"):
        out.tight = both_inf | (np.isfinite(out.t_in) & (out.t_in - out.t_out <= TIGHT * out.et))
    return out


def t_of_hits(origins, dirs, hits):
    """The ray parameter of a returned point, (h - o) . d / |d|^2 in float64 (0 for d = 0), and the rounding `s` of forming h = fl(o + fl(t d)) in
    fp32 as seen through that projection: each component of h is off by at most u (|t d_i| + |h_i|), so t by at most u (|t| |d| + |h|) / |d|."""
    o, d, h = (np.asarray(x, np.float64).reshape(-1, 3) for x in (origins, dirs, hits))
    dd = _dot(d, d)
    with np.errstate(all="ignore"):
        t = np.where(dd > 0, _dot(h - o, d) / np.where(dd > 0, dd, 1.0), 0.0)
        s = np.where(dd > 0, 1.01 * U * (np.abs(t) * np.sqrt(dd) + np.linalg.norm(h, axis=1)) / np.sqrt(np.where(dd > 0, dd, 1.0)), 0.0)
    return t, s


# ---------------------------------------------------------------------------------------------- quaternions (xyzw), float64
def quat_apply64(q, b):
    """b + w t + xyz x t, t = 2 xyz x b: the kernels' formula (lg_device.h), which is what an fp32 quaternion that is unit only to rounding asks for"""
    q, b = np.asarray(q, np.float64), np.asarray(b, np.float64)
    t = 2.0 * np.cross(q[..., :3], b)
    return b + q[..., 3:4] * t + np.cross(q[..., :3], t)


def quat_apply_err(q, b, q_rel=0.0):
    """Norm of the componentwise fp32 rounding bound of quat_apply (module docstring); q_rel: relative error of q's own components"""
    q, b = np.asarray(q, np.float64), np.asarray(b, np.float64)
    shape = np.broadcast_shapes(q.shape[:-1], b.shape[:-1])
    x = np.abs(np.broadcast_to(q[..., :3], shape + (3,))).reshape(-1, 3)
    w = np.abs(np.broadcast_to(q[..., 3:4], shape + (1,))).reshape(-1, 1)
    bb = np.abs(np.broadcast_to(b, shape + (3,))).reshape(-1, 3)
    qs = np.broadcast_to(q, shape + (4,)).reshape(-1, 4)
    bs = np.broadcast_to(b, shape + (3,)).reshape(-1, 3)
    t = 2.0 * np.cross(qs[:, :3], bs)
    A = 2.0 * _abscross(x, bb)
    dt = U * (A + np.abs(t))                                                  # two products and their difference (x 2 is exact)
    c = np.cross(qs[:, :3], t)
    dc = _abscross(x, dt) + U * (_abscross(x, np.abs(t)) + np.abs(c))
    s1 = bs + qs[:, 3:4] * t
    e = 1.01 * (w * dt + U * np.abs(qs[:, 3:4] * t) + U * np.abs(s1) + dc + U * np.abs(s1 + c)) + 2 * q_rel * (w * A + _abscross(x, A))
    return np.linalg.norm(e, axis=1).reshape(shape)


def quat_mul64(a, b, with_bound=False):
    """Isaac Gym's xyzw product as the depth kernel forms it; the bound: no entry is more than 7 roundings deep (a sum of two operands 1, a product 1, xx two
    sums, qq one (x 0.5 is exact), the result two): 8 u (sum of the absolute values of the five products)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    x1, y1, z1, w1 = (a[..., i] for i in range(4))
    x2, y2, z2, w2 = (b[..., i] for i in range(4))
    ww, yy, zz = (z1 + x1) * (x2 + y2), (w1 - y1) * (w2 + z2), (w1 + y1) * (w2 - z2)
    m = (z1 - x1) * (x2 - y2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + m)
    r = [(x1 + w1) * (x2 + w2), (w1 - x1) * (y2 + z2), (z1 + y1) * (w2 - x2), (z1 - y1) * (y2 - z2)]
    out = np.stack([qq - xx + r[0], qq - yy + r[1], qq - zz + r[2], qq - ww + r[3]], axis=-1)
    if not with_bound:
        return out
    S = np.abs(ww) + np.abs(yy) + np.abs(zz) + np.abs(m)
    return out, 8 * U * np.stack([S + np.abs(k) for k in r], axis=-1)


# ---------------------------------------------------------------------------------------------- the ray-caster sensor
@dataclass
class RaycasterRef:
    o: np.ndarray; d: np.ndarray            # (N, R, 3) float64 rays
    o_err: np.ndarray; d_err: np.ndarray    # (N, R) what the kernel's fp32 rays may be off by
    bounds: RayBounds                       # over the N * R rays
    hit_lo: np.ndarray; hit_hi: np.ndarray  # (N, R, 3) the returned point (the ray's end point on a miss)
    dist_lo: np.ndarray; dist_hi: np.ndarray  # (N, R) the distance row


def sensor_rays(root_states, pattern_o, pattern_d, yaw_only):
    rs = np.asarray(root_states, np.float32).astype(np.float64)
    po, pd = np.asarray(pattern_o, np.float32).astype(np.float64), np.asarray(pattern_d, np.float32).astype(np.float64)
    q = rs[:, 3:7].copy()
    q_rel = 0.0
    if yaw_only:
        q[:, :2] = 0.0
        q /= np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-9)
        q_rel = 3 * U                       # z^2 + w^2 (relative 2u), sqrt (u + u), the division (u): 3u on each component
    pos = rs[:, None, 0:3]
    rot_o = quat_apply64(q[:, None, :], po[None])
    o = rot_o + pos
    d = quat_apply64(q[:, None, :], pd[None])
    o_err = quat_apply_err(q[:, None, :], po[None], q_rel) + 1.01 * U * np.linalg.norm(o, axis=2)
    d_err = quat_apply_err(q[:, None, :], pd[None], q_rel)
    return o, d, o_err, d_err, rs[:, 0:3]


def raycaster_reference(vertices, triangles, root_states, pattern_o, pattern_d, max_dist, yaw_only):
    """Rounding carried beyond the bounds on t: the point h = fl(o + fl(t d)) is within o_err + t d_err + u (t |d| + |h|) of the float64 one; the distance
    |h - pos| adds u (|h| + |pos|) for the difference and 3u of itself for the norm; the row 1 - clip(dist / max_dist) adds 3u (division, clip, difference)."""
    o, d, o_err, d_err, pos = sensor_rays(root_states, pattern_o, pattern_d, yaw_only)
    N, R = o.shape[:2]
    md = float(np.float32(max_dist))
    rb = ray_bounds(vertices, triangles, o.reshape(-1, 3), d.reshape(-1, 3), max_dist, o_err.reshape(-1), d_err.reshape(-1))
    t_lo = np.minimum(rb.t_out, md).reshape(N, R)           # a miss returns the point at max_dist
    t_hi = np.minimum(rb.t_in, md).reshape(N, R)
    dn = np.linalg.norm(d, axis=2)
    ends = np.stack([o + t_lo[..., None] * d, o + t_hi[..., None] * d])
    herr = o_err + md * d_err + 1.01 * U * (md * dn + np.abs(ends).max(0).sum(2))
    hit_lo, hit_hi = ends.min(0) - herr[..., None], ends.max(0) + herr[..., None]
    c = o - pos[:, None, :]
    g = lambda t: np.linalg.norm(c + t[..., None] * d, axis=2)
    with np.errstate(all="ignore"):
        tstar = np.clip(-(c * d).sum(2) / np.maximum(dn * dn, 1e-300), t_lo, t_hi)
    d_min, d_max = g(tstar), np.maximum(g(t_lo), g(t_hi))
    ed = herr + 1.01 * U * (np.abs(ends).max(0).sum(2) + np.abs(pos).sum(1)[:, None]) + 3 * U * d_max
    row_hi = 1.0 - np.clip((d_min - ed) / md, 0.0, 1.0) + 3 * U
    row_lo = 1.0 - np.clip((d_max + ed) / md, 0.0, 1.0) - 3 * U
    may_miss, must_miss = ~rb.must_hit.reshape(N, R), rb.must_miss.reshape(N, R)
    row_lo = np.where(may_miss, 0.0, np.maximum(row_lo, 0.0))
    row_hi = np.where(must_miss, 0.0, np.minimum(row_hi, 1.0))
    return RaycasterRef(o, d, o_err, d_err, rb, hit_lo, hit_hi, row_lo, row_hi)


# ---------------------------------------------------------------------------------------------- the depth camera
def bicubic_taps(n_in, n_out, a=-0.75, align_corners=False):
    """Source index of tap -1 (unclamped) and the four Keys weights of every output index, float64"""
    i = np.arange(n_out, dtype=np.float64)
    if align_corners:
        f = i * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    else:
        f = (i + 0.5) * (n_in / n_out) - 0.5
    i0 = np.floor(f)
    t = f - i0

    def w(x):
        x = np.abs(x)
        return np.where(x <= 1, ((a + 2) * x - (a + 3)) * x * x + 1, np.where(x < 2, ((a * x - 5 * a) * x + 8 * a) * x - 4 * a, 0.0))
    return i0.astype(np.int64), np.stack([w(t - k) for k in (-1, 0, 1, 2)], axis=1), f


def bicubic64(img, RW, RH, a=-0.75, align_corners=False, clamp=True):
    """(..., H, W) -> (..., RH, RW); clamp=False reads zeros outside the image (a fault of the power tests)"""
    H, W = img.shape[-2:]
    ix, wx, _ = bicubic_taps(W, RW, a, align_corners)
    iy, wy, _ = bicubic_taps(H, RH, a, align_corners)
    out = np.zeros(img.shape[:-2] + (RH, RW))
    for m in range(4):
        yy = iy - 1 + m
        for k in range(4):
            xx = ix - 1 + k
            src = img[..., np.clip(yy, 0, H - 1)[:, None], np.clip(xx, 0, W - 1)[None, :]]
            if not clamp:
                src = src * (((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :])
            out += wy[:, m][:, None] * wx[:, k][None, :] * src
    return out


@dataclass
class DepthRef:
    cam_pos: np.ndarray; cam_pos_err: np.ndarray      # (N, 3), (N,)
    cam_rot: np.ndarray; cam_rot_err: np.ndarray      # (N, 4), (N, 4)
    bounds: RayBounds                                  # over N * H * W rays
    src_lo: np.ndarray; src_hi: np.ndarray            # (N, H, W) clipped depth before the resize
    lo: np.ndarray; hi: np.ndarray                    # (N, RH, RW) the new frame, from the ray bounds alone
    round: np.ndarray                                  # (N, RH, RW) the fp32 rounding of resize and normalisation, to be allowed on either side
    src_tight: np.ndarray                              # (N, RH, RW) all 16 source pixels come from tight rays
    old: np.ndarray                                    # (N, buffer_len - 1, RH, RW) what the older frames of a shifted FIFO must equal bit for bit
    init: np.ndarray                                   # (N,) ep_len <= 1: every frame of the FIFO is the new one


def depth_reference(vertices, triangles, cfg, root_states, pattern_dirs, ep_len, env_noise, buffer_before, mount_quat, pose=None):
    """cfg: original (W, H), resized (RW, RH), near_clip, far_clip, position, buffer_len.  pose = (camera_pos, camera_rot) as fp32 arrays: the rays are formed
    from THAT pose (the device's own, which the caller holds to cam_pos / cam_rot here within their bounds) and only quat_apply's rounding widens them;
    without it from the float64 pose, widened by the pose's bounds (a direction moves by at most 8 |dq| |b|: t, w t and xyz x t are each bilinear in q).

    Stated fp32 terms.  depth = -(t |d|): 4u far (norm 2, product 1, and 1 for the sum with the noise) + t d_err.  Resize: f = (i + 0.5) s - 0.5 is off by 3u |f|
    (s, the product, the difference), a weight by 1.5 times that (|w'| <= 1.35) plus 4u of its own evaluation; the weights of an axis sum to 1, so what their
    errors move is the spread r of the 16 sources around their centre c: (sum_x |dw| sum_y |w| + sum_y |dw| sum_x |w|) r + 32u |c|; the sum itself is 10
    roundings deep: 10u sum |w| |src|.  Normalisation: 3u (|v| + near) / (far - near) + u."""
    W, H = cfg.original
    RW, RH = cfg.resized
    near, far = float(np.float32(cfg.near_clip)), float(np.float32(cfg.far_clip))
    rs = np.asarray(root_states, np.float32).astype(np.float64)
    N = len(rs)
    bq = rs[:, 3:7]
    off = np.asarray(np.float32(getattr(cfg, "position", [0.0, 0.0, 0.0])), np.float64)
    rot_off = quat_apply64(bq, off[None])
    cpos = rs[:, 0:3] + rot_off
    cpos_err = quat_apply_err(bq, off[None]) + 1.01 * U * np.linalg.norm(cpos, axis=1)
    crot, crot_err = quat_mul64(bq, np.asarray(np.float32(mount_quat), np.float64)[None], with_bound=True)
    pd = np.asarray(pattern_dirs, np.float32).astype(np.float64).reshape(-1, 3)
    if pose is None:
        o, q = cpos, crot
        o_err = np.broadcast_to(cpos_err[:, None], (N, len(pd)))
        extra = 8 * np.linalg.norm(crot_err, axis=1)[:, None] * np.linalg.norm(pd, axis=1)[None]
    else:
        o, q = np.asarray(pose[0], np.float32).astype(np.float64), np.asarray(pose[1], np.float32).astype(np.float64)
        o_err, extra = np.zeros((N, len(pd))), 0.0
    d = quat_apply64(q[:, None, :], pd[None])
    d_err = quat_apply_err(q[:, None, :], pd[None]) + extra
    oo = np.broadcast_to(o[:, None, :], d.shape)
    rb = ray_bounds(vertices, triangles, oo.reshape(-1, 3), d.reshape(-1, 3), far, np.asarray(o_err).reshape(-1), d_err.reshape(-1))
    dn = np.linalg.norm(d, axis=2).reshape(-1)
    noise = np.zeros(N) if env_noise is None else np.asarray(env_noise, np.float32).astype(np.float64)
    nz = np.repeat(noise, len(pd))
    r0 = lambda t: 4 * U * far + d_err.reshape(-1) * np.minimum(t, far)      # (|d| is off by at most d_err)
    with np.errstate(invalid="ignore"):
        dep_lo = np.where(np.isfinite(rb.t_in), -rb.t_in * dn - r0(rb.t_in), -far)       # may miss: -far
        dep_hi = np.where(np.isfinite(rb.t_out), -rb.t_out * dn + r0(rb.t_out), -far)
    src_lo = np.clip(dep_lo + nz, -far, -near).reshape(N, H, W)
    src_hi = np.clip(dep_hi + nz, -far, -near).reshape(N, H, W)
    tight_src = rb.tight.reshape(N, H, W)
    if RW == W and RH == H:
        lo, hi, rnd, st = src_lo, src_hi, np.zeros_like(src_lo), tight_src
    else:
        ix, wx, fx = bicubic_taps(W, RW)
        iy, wy, fy = bicubic_taps(H, RH)
        lo, hi, sabs = np.zeros((N, RH, RW)), np.zeros((N, RH, RW)), np.zeros((N, RH, RW))
        vmin, vmax = np.full((N, RH, RW), np.inf), np.full((N, RH, RW), -np.inf)
        st = np.ones((N, RH, RW), bool)
        for m in range(4):
            yy = np.clip(iy - 1 + m, 0, H - 1)[:, None]
            for k in range(4):
                xx = np.clip(ix - 1 + k, 0, W - 1)[None, :]
                w = (wy[:, m][:, None] * wx[:, k][None, :])[None]
                a_lo, a_hi = src_lo[:, yy, xx], src_hi[:, yy, xx]
                lo += np.where(w >= 0, w * a_lo, w * a_hi)
                hi += np.where(w >= 0, w * a_hi, w * a_lo)
                sabs += np.abs(w) * np.maximum(np.abs(a_lo), np.abs(a_hi))
                vmin, vmax = np.minimum(vmin, a_lo), np.maximum(vmax, a_hi)
                st &= tight_src[:, yy, xx]
        dwx = 1.5 * 3 * U * (np.abs(fx) + 0.5) + 4 * U
        dwy = 1.5 * 3 * U * (np.abs(fy) + 0.5) + 4 * U
        swx, swy = np.abs(wx).sum(1), np.abs(wy).sum(1)
        spread = (4 * dwx[None, :] * swy[:, None] + 4 * dwy[:, None] * swx[None, :])[None]
        rnd = spread * 0.5 * (vmax - vmin) + 32 * U * 0.5 * np.abs(vmax + vmin) + 10 * U * sabs
    scale = far - near
    n_lo, n_hi = (-hi - near) / scale - 0.5, (-lo - near) / scale - 0.5
    rnd = rnd / scale + 3 * U * (np.maximum(np.abs(lo), np.abs(hi)) + near) / scale + U
    before = np.asarray(buffer_before)
    init = np.asarray(ep_len).reshape(-1) <= 1
    return DepthRef(cpos, cpos_err, crot, crot_err, rb, src_lo, src_hi, n_lo, n_hi, rnd, st, before[:, 1:].copy(), init)


# ---------------------------------------------------------------------------------------------- what the tests assert (CPU restatement and device alike)
def cast_violations(rb, origins, dirs, hits, found, max_dist):
    """lg_raycast_mesh against `rb`, per ray: t outside [t_out - s, t_in + s] (a miss is inf), found not exact on a tight ray, a returned point off its ray
    (componentwise 2u (|t d_i| + |h_i|) next to the float64 o + t d, t the projection of the point itself), a miss not at o + max_dist d."""
    o, d, h = (np.asarray(x, np.float64).reshape(-1, 3) for x in (origins, dirs, hits))
    f = np.asarray(found).reshape(-1).astype(bool)
    md = float(np.float32(max_dist))
    tk, s = t_of_hits(o, d, h)
    tk = np.where(f, tk, md)
    t_eff = np.where(f, tk, np.inf)
    with np.errstate(invalid="ignore"):
        bad_t = (t_eff > rb.t_in + s) | (t_eff < rb.t_out - s)
    bad_found = rb.tight & (f != rb.must_hit)
    pt = o + tk[:, None] * d
    off_ray = (np.abs(h - pt) > 2.02 * U * (np.abs(tk[:, None] * d) + np.abs(h)) + s[:, None] * np.abs(d) + 1e-30).any(1)
    return dict(t=bad_t, found=bad_found, point=off_ray), np.where(f, tk, np.inf)


def raycaster_violations(ref, hits, found, rows):
    h, f, r = np.asarray(hits, np.float64), np.asarray(found).astype(bool), np.asarray(rows, np.float64)
    N, R = f.shape
    tight, must_hit = ref.bounds.tight.reshape(N, R), ref.bounds.must_hit.reshape(N, R)
    bad_found = (tight & (f != must_hit)) | (f & ref.bounds.must_miss.reshape(N, R)) | (~f & must_hit)
    bad_hit = ((h < ref.hit_lo) | (h > ref.hit_hi)).any(2)
    bad_row = (r < ref.dist_lo) | (r > ref.dist_hi) | (~f & (r != 0.0))
    return dict(found=bad_found, point=bad_hit, row=bad_row)


def depth_violations(ref, frame):
    """pixels of the new frame outside [lo - round, hi + round], and where inside the interval each pixel sits (0 = lo, 1 = hi; widened interval)"""
    x = np.asarray(frame, np.float64)
    lo, hi = ref.lo - ref.round, ref.hi + ref.round
    return (x < lo) | (x > hi), (x - lo) / np.maximum(hi - lo, 1e-300)
