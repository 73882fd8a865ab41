"""CPU: the float64 ray bounds of tests/ray_reference.py are right, tight and sharp enough to catch a wrong kernel -- before tests/test_hip_ray_reference.py
holds the device to them.

  known answers   of the reference itself: a box from above, the unit icosphere from outside and from its centre (t within the facet sagitta), one triangle
                  from both sides, through a vertex, across and along an edge, a ray that starts on the face, a ray that ends exactly at max_dist
  bicubic         the float64 Keys resize against torch's float64 `interpolate(mode="bicubic")`: down, identity, up
  oracle inside   the CPU oracle's fp32 brute-force scan (`lgo_raycast_bruteforce`) lies inside the bounds on EVERY ray of every set on every mesh of
                  tests/ray_cases.py (this is what confirms K; it is never tuned against a kernel)
  tight shares    conditions on the inputs: >= 98 % of each random / grazing / sensor set tight, >= 50 % of each deliberately degenerate one, >= 97 % of the
                  output pixels of each depth case with hi - lo <= 1e-5
  power           faults applied to a numpy fp32 restatement of the scan and of the sensor / depth arithmetic (tests/ray_cases.py): each breaks the bounds
                  on >= 10 rays or pixels of the set named next to it, and the faultless restatement breaks none"""
import numpy as np
import pytest
import torch

from extended_legged_gym_amd.utils.depth_camera import mount_quat_as_reference
from extended_legged_gym_amd.utils.ray_caster import PatternType, RayCasterPatternCfg
from oracle.oracle_lib import raycast_bruteforce
from tests import ray_cases as rc
from tests import ray_reference as rr
from tests.test_sensors_host import box_mesh, icosphere

_CACHE = {}


def mesh_case(name):
    """(vertices, triangles, ray sets, bounds per set), computed once"""
    if name not in _CACHE:
        v, t = rc.MESHES[name]()
        sets = rc.ray_sets(v, exact_t=lambda o, d: rr.ray_bounds(v, t, o, d, 100.0).t_in)
        _CACHE[name] = (v, t, sets, {k: rr.ray_bounds(v, t, o, d, rc.MAX_DIST) for k, (o, d) in sets.items()})
    return _CACHE[name]


def strip_case(cells):
    key = ("strip", cells)
    if key not in _CACHE:
        v, t = rc.strip_mesh(cells)
        sets = {k: x for k, x in rc.ray_sets(v, m=80).items() if k in ("random_down", "grazing", "vertical", "on_lines")}
        _CACHE[key] = (v, t, sets, {k: rr.ray_bounds(v, t, o, d, rc.MAX_DIST) for k, (o, d) in sets.items()})
    return _CACHE[key]


def one(v, t, o, d, max_dist):
    return rr.ray_bounds(v, t, np.array([o], np.float32), np.array([d], np.float32), max_dist)


# ---------------------------------------------------------------------------------------------- known answers
def test_known_answers_box_and_icosphere():
    v, t = box_mesh(1.0, 1.0, 0.5)
    b = one(v, t, [0.3, -0.2, 5.0], [0, 0, -1.0], 100.0)
    assert b.tight[0] and abs(b.t_in[0] - 4.5) < 1e-5 and abs(b.t_out[0] - 4.5) < 1e-5
    b = one(v, t, [0.0, 0.0, 5.0], [0, 0, -1.0], 100.0)                    # on the diagonal both top faces share: still decided
    assert b.tight[0] and abs(b.t_in[0] - 4.5) < 1e-5
    assert one(v, t, [3.0, 0.0, 5.0], [0, 0, -1.0], 100.0).must_miss[0]
    assert one(v, t, [0.3, -0.2, 5.0], [0, 0, -1.0], 4.0).must_miss[0]      # shorter than the way to the top
    vi, ti = icosphere(2)
    tri = vi[ti].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    sag = 1.0 - np.abs((tri[:, 0] * n).sum(1) / np.linalg.norm(n, axis=1)).min()     # the deepest facet below the unit sphere
    assert 0 < sag < 0.03
    rng = np.random.default_rng(0)
    u = rng.normal(size=(200, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = rng.uniform(1.5, 3.0, 200)
    o = (u * r[:, None]).astype(np.float32)
    b = rr.ray_bounds(vi, ti, o, (-u).astype(np.float32), 10.0)
    rn = np.linalg.norm(o.astype(np.float64), axis=1)
    assert b.must_hit.all() and (b.t_out >= rn - 1 - 1e-5).all() and (b.t_in <= rn - 1 + sag + 1e-5).all() and b.tight.mean() > 0.98
    b = rr.ray_bounds(vi, ti, np.zeros((200, 3), np.float32), u.astype(np.float32), 10.0)
    assert b.must_hit.all() and (b.t_out >= 1 - sag - 1e-5).all() and (b.t_in <= 1 + 1e-5).all()
    assert rr.ray_bounds(vi, ti, np.zeros((200, 3), np.float32), u.astype(np.float32), 0.9).must_miss.all()


def test_known_answers_single_triangle():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    t = np.array([[0, 1, 2]], np.int32)
    for z, dz in ((1.0, -1.0), (-1.0, 1.0)):                                  # two-sided
        b = one(v, t, [0.25, 0.25, z], [0, 0, dz], 5.0)
        assert b.tight[0] and abs(b.t_in[0] - 1.0) < 5e-6 and b.face_in[0] == 0
    for x, y in ((0.0, 0.0), (1.0, 0.0), (0.5, 0.0), (0.5, 0.5), (-5e-6, 0.3)):   # through vertices, across edges, inside the band: must hit
        b = one(v, t, [x, y, 1.0], [0, 0, -1.0], 5.0)
        assert b.must_hit[0] and b.tight[0], (x, y)
    for x, y in ((-2e-5, 0.3), (0.3, -2e-5), (0.50002, 0.50002)):             # beyond the band: must miss
        assert one(v, t, [x, y, 1.0], [0, 0, -1.0], 5.0).must_miss[0], (x, y)
    b = one(v, t, [-1.0, 0.0, 0.0], [1.0, 0, 0], 5.0)                          # ALONG an edge, in the plane: undecided, and no earlier than the triangle
    assert not b.must_hit[0] and not b.tight[0] and 0.99 <= b.t_out[0] <= 1.0
    assert one(v, t, [-1.0, 0.0, 0.01], [1.0, 0, 0], 5.0).must_miss[0]         # ... a centimetre above the plane: a miss
    vt, tt = rc.triangle_mesh()                                                # starts ON a tilted face (to fp32 rounding): t = +-1e-8 may be accepted, need not be
    b = one(vt, tt, vt.astype(np.float64).mean(0), [0.1, 0.2, -1.0], 5.0)
    assert not b.must_hit[0] and b.t_out[0] == 0.0 and not b.tight[0]
    assert one(vt, tt, vt.astype(np.float64).mean(0) + [0, 0, 1e-4], [0.1, 0.2, -1.0], 5.0).tight[0]
    b = one(v, t, [0.25, 0.25, 2.0], [0, 0, -1.0], 2.0)                        # ends exactly on it
    assert not b.must_hit[0] and abs(b.t_out[0] - 2.0) < 5e-6 and not b.tight[0]
    assert one(v, t, [0.25, 0.25, 2.0], [0, 0, -1.0], 2.0002).tight[0] and one(v, t, [0.25, 0.25, 2.0], [0, 0, -1.0], 1.9998).must_miss[0]
    b = one(v, t, [0.25, 0.25, 1.0], [0, 0, -4.0], 5.0)                        # t is in units of |d|
    assert b.tight[0] and abs(b.t_in[0] - 0.25) < 5e-6
    b = one(v, t, [0.25, 0.25, 1.0], [0, 0, 0.0], 5.0)                         # d = 0
    assert b.must_miss[0] and not b.must_hit[0] and b.tight[0]
    vz = np.vstack([v, [[2.0, 2.0, 0.0], [2.0, 2.0, 0.0]]]).astype(np.float32)  # a zero-area face is skipped
    assert one(vz, np.array([[0, 1, 2], [2, 3, 4]], np.int32), [2.0, 2.0, 1.0], [0, 0, -1.0], 5.0).must_miss[0]


@pytest.mark.parametrize("shape", [((60, 30), (56, 28)), ((7, 5), (7, 5)), ((9, 9), (13, 11)), ((64, 1), (32, 1))])
def test_bicubic_is_torchs_in_float64(shape):
    (W, H), (RW, RH) = shape
    img = np.random.default_rng(1).normal(size=(3, H, W))
    want = torch.nn.functional.interpolate(torch.from_numpy(img)[:, None], size=(RH, RW), mode="bicubic", align_corners=False)[:, 0].numpy()
    got = rr.bicubic64(img, RW, RH)
    assert np.abs(got - want).max() < 1e-13
    if (W, H) == (RW, RH):
        assert np.array_equal(got, img)


# ---------------------------------------------------------------------------------------------- the oracle inside the bounds; tight shares
def _assert_oracle_inside(v, t, sets, bounds, tag):
    for k, (o, d) in sets.items():
        h, f = raycast_bruteforce(v, t, o, d, rc.MAX_DIST)
        bad, _ = rr.cast_violations(bounds[k], o, d, h, f, rc.MAX_DIST)
        for what, m in bad.items():
            assert not m.any(), (tag, k, what, np.nonzero(m)[0][:5])


@pytest.mark.parametrize("name", list(rc.MESHES))
def test_oracle_scan_lies_inside_the_bounds_on_every_ray(name):
    v, t, sets, bounds = mesh_case(name)
    assert "near_maxd" in sets and len(sets) == 10
    _assert_oracle_inside(v, t, sets, bounds, name)


@pytest.mark.parametrize("cells", [5997, 5998])
def test_oracle_scan_lies_inside_the_bounds_on_the_strips(cells):
    _assert_oracle_inside(*strip_case(cells), cells)


@pytest.mark.parametrize("name", list(rc.MESHES))
def test_tight_shares_of_the_ray_sets(name):
    v, t, sets, bounds = mesh_case(name)
    for k, b in bounds.items():
        share = b.tight.mean()
        print(name, k, "tight", round(float(share), 4))
        assert share >= (0.5 if k in rc.DEGENERATE_SETS else 0.98), (name, k, share)
    md = float(np.float32(rc.MAX_DIST))
    near = bounds["near_maxd"]
    t_mid = np.where(near.must_hit, near.t_in, near.t_out)
    assert (np.abs(t_mid[np.isfinite(t_mid)] - md) < 1.2e-4).mean() > 0.3      # the set does what its name says: hits placed within 1e-4 of max_dist


SENSORS = {"single": RayCasterPatternCfg(pattern_type=PatternType.SINGLE_RAY, single_ray_direction=[0.6, 0.0, -0.8]),
           "spherical48": RayCasterPatternCfg(pattern_type=PatternType.SPHERICAL2, spherical2_num_points=48),
           "cone65": RayCasterPatternCfg(pattern_type=PatternType.CONE, cone_num_rays=65, cone_angle=50.0)}
SENSOR_OFFSET, SENSOR_MAX = [0.3, 0.0, 0.05], 2.5


def sensor_case(pattern, yaw_only):
    key = ("sensor", pattern, yaw_only)
    if key not in _CACHE:
        v, t = mesh_case("hf24")[:2]
        root = rc.sensor_roots(v)
        po, pd = SENSORS[pattern].create_pattern("cpu")
        po = (po + torch.tensor(SENSOR_OFFSET)).numpy()
        _CACHE[key] = (v, t, root, po, pd.numpy(), rr.raycaster_reference(v, t, root, po, pd.numpy(), SENSOR_MAX, yaw_only))
    return _CACHE[key]


@pytest.mark.parametrize("yaw_only", [True, False])
def test_sensor_restatement_inside_and_tight(yaw_only):
    tight = []
    for pattern in SENSORS:
        v, t, root, po, pd, ref = sensor_case(pattern, yaw_only)
        h, f, rows = rc.raycaster32(v, t, root, po, pd, SENSOR_MAX, yaw_only)
        for what, m in rr.raycaster_violations(ref, h, f, rows).items():
            assert not m.any(), (pattern, what)
        tight.append(ref.bounds.tight)
        width = (ref.dist_hi - ref.dist_lo)[ref.bounds.tight.reshape(ref.dist_lo.shape)]
        assert width.max() < 1e-4, (pattern, width.max())                       # a tight ray pins its distance row (to 1e-4 of the range, whatever its angle)
    share = np.concatenate(tight).mean()
    print("sensor rays tight", share)
    assert share >= 0.98


def depth_case(name, pose_from_restatement=True):
    key = ("depth", name, pose_from_restatement)
    if key not in _CACHE:
        v, t = mesh_case("hf24")[:2]
        original, resized, blen, ep_len, noise = rc.DEPTH_CASES[name]
        cfg = rc.depth_cfg(original, resized, blen)
        root = rc.depth_roots(v)
        pdirs = rc.pattern_dirs(cfg)
        before = np.random.default_rng(9).uniform(-0.5, 0.5, size=(3, blen, resized[1], resized[0])).astype(np.float32)
        mount = mount_quat_as_reference(cfg)
        args = (v, t, cfg, root, pdirs, np.array(ep_len), noise, before, mount)
        cpos, cq, buf = rc.depth32(*args)
        ref = rr.depth_reference(*args, pose=(cpos, cq) if pose_from_restatement else None)
        _CACHE[key] = (args, (cpos, cq, buf), ref)
    return _CACHE[key]


@pytest.mark.parametrize("name", list(rc.DEPTH_CASES))
def test_depth_restatement_inside_and_tight(name):
    args, (cpos, cq, buf), ref = depth_case(name)
    assert (np.linalg.norm(cpos - ref.cam_pos, axis=1) <= ref.cam_pos_err).all() and (np.abs(cq - ref.cam_rot) <= ref.cam_rot_err).all()
    bad, _ = rr.depth_violations(ref, buf[:, -1])
    assert not bad.any(), (name, int(bad.sum()))
    share = ((ref.hi - ref.lo) <= 1e-5).mean()
    print(name, "pixels with hi - lo <= 1e-5:", share, "largest rounding term", ref.round.max())
    assert share >= 0.97, (name, share)
    if name == "shipped":                                                     # the camera on the lattice corner sees the mesh; the image is not flat
        assert buf[2, -1].std() > 0.01 and buf[0, -1].std() > 0.01
    if args[6] is not None:                                                   # the noise takes some pixels through both clips
        assert (ref.src_hi == 0.0).any() and (ref.src_lo == -2.0).any()


# ---------------------------------------------------------------------------------------------- power
def _cast_broken(name, k, **faults):
    if "+" in k:                                                              # a union of sets
        return sum(_cast_broken(name, part, **faults) for part in k.split("+"))
    v, t, sets, bounds = mesh_case(name)
    o, d = sets[k]
    h, f = rc.cast32(v, t, o, d, rc.MAX_DIST, **faults)
    bad, _ = rr.cast_violations(bounds[k], o, d, h, f, rc.MAX_DIST)
    return int((bad["t"] | bad["found"] | bad["point"]).sum())


def test_power_faultless_scan_breaks_nothing():
    for name in rc.MESHES:
        for k in mesh_case(name)[2]:
            assert _cast_broken(name, k) == 0, (name, k)


def _column_faces(name, col):
    v, t = mesh_case(name)[:2]
    xs = np.unique(v[:, 0])
    cx = v[t][:, :, 0].mean(1)
    return (cx > xs[col]) & (cx < xs[col + 1])


@pytest.mark.parametrize("fault,name,k", [
    (dict(drop="column"), "hf24", "random_down+vertical+parallel+under_up"),     # one cell column's faces removed (1 of 23: ~2 % of the hits)
    (dict(first=True), "hf24", "grazing"),                  # the first hit found instead of the nearest
    (dict(cull=True), "hf24", "under_up"),                  # one-sided culling
    (dict(band=-1e-5), "hf24", "on_lines"),                 # shrunken triangles: cracks on lattice lines
    (dict(md_scale=0.999), "hf24", "near_maxd"),            # max_dist applied at 0.999 x
    (dict(miss_at_origin=True), "hf24", "outside"),         # a miss's end point at the origin
])
def test_power_scan_faults(fault, name, k):
    if fault.get("drop") == "column":
        fault = dict(drop=_column_faces(name, 11))
    n = _cast_broken(name, k, **fault)
    print(fault if "drop" not in fault else "column 11 dropped", name, k, "rays outside the bounds:", n)
    assert n >= 10


@pytest.mark.parametrize("fault,what", [(dict(from_origin=True), "row"), (dict(ignore_yaw_only=True), "point"), (dict(miss_at_origin=True), "point")])
def test_power_sensor_faults(fault, what):
    v, t, root, po, pd, ref = sensor_case("spherical48", True)
    h, f, rows = rc.raycaster32(v, t, root, po, pd, SENSOR_MAX, True, **fault)
    n = int(rr.raycaster_violations(ref, h, f, rows)[what].sum())
    print(fault, "spherical48 / yaw-only:", what, "outside the intervals:", n)
    assert n >= 10


@pytest.mark.parametrize("fault,name", [
    (dict(swap_mul=True), "shipped"), (dict(a=-0.5), "shipped"), (dict(align_corners=True), "shipped"), (dict(clamp=False), "shipped"),
    (dict(unwritten="row"), "upsample"), (dict(unwritten="col"), "upsample"), (dict(noise_after_clip=True), "identity"),
    (dict(noise_after_clip=True), "upsample")])
def test_power_depth_faults(fault, name):
    args, _, ref = depth_case(name, pose_from_restatement="swap_mul" not in fault)      # (the swapped product is held by the pose-free reference)
    cpos, cq, buf = rc.depth32(*args, **fault)
    bad, _ = rr.depth_violations(ref, buf[:, -1])
    print(fault, name, "pixels outside their intervals:", int(bad.sum()))
    assert bad.sum() >= 10
    if "swap_mul" in fault:
        good = rc.depth32(*args)
        assert not rr.depth_violations(ref, good[2][:, -1])[0].any()           # the pose-free reference holds the faultless frame too
        assert (np.abs(cq - ref.cam_rot) > ref.cam_rot_err).any()


def test_power_fifo_shifted_the_wrong_way():
    args, (_, _, good), ref = depth_case("upsample")                           # buffer_len 3; ep_len (1, 2, 0): env 1 shifts
    assert ref.init.tolist() == [True, False, True]
    assert np.array_equal(good[~ref.init][:, :-1], ref.old[~ref.init])
    bad = rc.depth32(*args, fifo_wrong_way=True)[2]
    assert (bad[~ref.init][:, :-1] != ref.old[~ref.init]).sum() >= 10
