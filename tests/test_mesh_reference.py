"""CPU: the float64 closest-point reference of tests/mesh_reference.py (the checker of tests/test_hip_mesh_sdf_reference.py)
against known answers and against the fp32 brute-force scan of the oracle."""
import numpy as np

from oracle.oracle_lib import sdf_bruteforce
from tests.mesh_reference import closest_point_f64, signed_reference
from tests.test_sensors_host import icosphere

TRI_V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
TRI_T = np.array([[0, 1, 2]])


def test_single_triangle_regions():
    pts = np.array([
        [0.25, 0.25, 0.5],     # above the interior
        [0.5, -0.3, 0.4],      # beyond edge ab (y = 0)
        [-0.3, 0.5, -0.4],     # beyond edge ac (x = 0)
        [0.8, 0.8, 0.0],       # beyond edge bc (x + y = 1)
        [-0.5, -0.5, 0.2],     # beyond vertex a
        [1.6, -0.2, 0.0],      # beyond vertex b
        [-0.1, 1.7, 0.3],      # beyond vertex c
        [0.2, 0.3, 0.0],       # on the surface
    ])
    want_q = np.array([[0.25, 0.25, 0], [0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0.2, 0.3, 0]])
    r = closest_point_f64(TRI_V, TRI_T, pts, 10.0)
    np.testing.assert_allclose(r.q, want_q, atol=1e-15)
    np.testing.assert_allclose(r.d, np.linalg.norm(pts - want_q, axis=1), atol=1e-15)
    assert r.d[-1] < 1e-15 and (r.face == 0).all()
    s = signed_reference(TRI_V, TRI_T, pts, 10.0)
    assert s.sign.tolist() == [1, 1, -1, 1, 1, 1, 1, 1]                     # (the normal is +z: the third point is below)
    assert s.sure.tolist() == [True, True, True, False, True, False, True, False]   # (in the plane: no side; on the surface: d = 0)


def test_beyond_max_dist_reports_no_face():
    r = closest_point_f64(TRI_V, TRI_T, [[0.25, 0.25, 2.0], [0.25, 0.25, 0.5]], 1.0)
    assert r.face.tolist() == [-1, 0] and abs(r.d[0] - 2.0) < 1e-15
    s = signed_reference(TRI_V, TRI_T, [[0.25, 0.25, 2.0]], 1.0)
    assert s.sdf[0] == 1.0 and not s.sure[0]


def test_zero_area_faces_are_skipped():
    v = np.vstack([TRI_V, [[0.0, 0.0, 1.0], [0.0, 0.0, 2.0]]])
    t = np.array([[0, 1, 2], [0, 3, 4]])                                     # the second face is a segment (zero area) up the z axis
    r = closest_point_f64(v, t, [[0.0, 0.0, 1.5]], 10.0)
    assert r.face[0] == 0 and abs(r.d[0] - 1.5) < 1e-15


def test_shared_edge_is_a_tie_and_the_outside_face_decides():
    # two faces of a roof share its ridge (x = 0, z = 1): a point above the ridge is equally close to both, and both say "outside"
    v = np.array([[0.0, 0, 1], [0, 1, 1], [-1, 0, 0], [1, 0, 0], [-1, 1, 0], [1, 1, 0]])
    t = np.array([[2, 0, 4], [0, 1, 4], [0, 3, 1], [3, 5, 1]])
    s = signed_reference(v, t, [[0.0, 0.5, 1.5]], 10.0)
    assert sorted(s.ref.band_faces(0).tolist()) == [1, 2]
    assert s.sign[0] == 1 and s.sure[0] and s.unique[0]


def test_icosphere_centre_is_inside():
    v, t = icosphere(3)
    s = signed_reference(v, t, [[0.0, 0, 0], [0, 0, 2.0], [0.3, -0.2, 0.1]], 10.0)
    assert -1.0 <= s.sdf[0] <= -0.98 and abs(s.sdf[1] - 1.0) < 0.01 and s.sdf[2] < -0.6
    # the centre is equally far from faces on opposite sides: the point of one with the normal of another gives either sign
    assert len(s.ref.band_faces(0)) > 2 and s.sure.tolist() == [False, True, True]


def test_agrees_with_the_fp32_oracle_on_the_rough_mesh():
    from tests.test_hip_sensors import rough_mesh
    v, t = rough_mesh()
    rng = np.random.default_rng(7)
    pts = np.column_stack([rng.uniform(-2.2, 2.2, 2000), rng.uniform(-2.2, 2.2, 2000), rng.uniform(-0.5, 1.0, 2000)]).astype(np.float32)
    s = signed_reference(v, t, pts, 0.8)
    s32, _ = sdf_bruteforce(v, t, pts, 0.8)
    near = s.ref.d < 0.8 - 1e-4
    assert near.mean() > 0.5
    np.testing.assert_allclose(np.abs(s32[near]), s.ref.d[near], atol=1e-5)
    assert (np.sign(s32[near & s.sure]) == s.sign[near & s.sure]).all()
    far = s.ref.d > 0.8 * (1 + 1e-4)
    assert (s32[far] == np.float32(0.8)).all()
