"""Capsule segments against the edges of a LATTICE mesh (TerrainObj OBJ files, TerrainConfined): the reference loads every collision cylinder as a capsule
(`asset.replace_cylinder_with_capsule = True`, legged_robot_config.py:171, legged_robot.py:741) on every terrain.  Opt-in here: `terrain.lattice_mesh_capsules`
-> `lg_set_lattice_capsules` (kernel: `lattice_caps_edges` of lg_physics.h, the physics_kernel instances with FEAT bit 2).

There is no oracle restatement of the lattice rule (oracle/ stays as it is).  What pins it instead:
* known answers -- a shank lowered onto a stair nosing between two of its spheres (the staircase of tests/test_mesh_capsules.py, with a flat strip along one
  edge that keeps its lattice even, written to an OBJ file and loaded through TerrainObj), and a shank or thigh pushed up into the step edge of a CEILING (the case a sign rule that only works facing up gets wrong);
* agreement with the grid-mesh path (`contact_detect_mesh<true>`), which the oracle pins (test_mesh_capsules.py), on the same staircase and states;
* what one env finds does not depend on the other envs of its wave; shanks lying on flat ground (no creases) and robots away from edges: on and off
  bit-identical; the fused rollout tail carries the same rule; config 3 and the hexapod stay finite and on the mesh.

CPU: the switch's plumbing and the kernel instances' register / LDS budgets.  GPU (`-m gpu`): the rest."""
import json
import os

import numpy as np
import pytest

from extended_legged_gym_amd import abi
from tests.test_mesh_capsules import R_SHANK, load_oracle, nosing_clearance, stairs_setup, stairs_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------------------------- CPU: plumbing
def test_switch_plumbing_and_refusals():
    """`terrain.lattice_mesh_capsules` exists (off by default), NativeSetup carries it, refuses it where it cannot act, and the entry point is declared and
    listed among the library's product symbols."""
    from extended_legged_gym_amd.envs.anymal_c.mixed_terrains.anymal_c_rough_config import AnymalCRoughCfg
    from extended_legged_gym_amd.envs.base.legged_robot_config import LeggedRobotCfg
    from extended_legged_gym_amd.envs.base.native_config import NativeSetup, load_robot_model
    from tests.helpers import sim_params_for
    assert LeggedRobotCfg.terrain.lattice_mesh_capsules is False
    assert AnymalCRoughCfg().terrain.lattice_mesh_capsules is False
    cfg, ter, s, model = stairs_setup(8)
    assert s.lattice_mesh_capsules is False
    # a height grid / plane is no lattice mesh
    cfg.terrain.lattice_mesh_capsules = True
    cfg.terrain.mesh_type = "heightfield"
    with pytest.raises(ValueError, match="triangle-mesh terrain"):
        NativeSetup(cfg, sim_params_for(cfg), model, terrain=ter, seed=0)
    # without capsules there are no segments
    cfg.terrain.mesh_type = "trimesh"
    cfg.asset.replace_cylinder_with_capsule = False
    with pytest.raises(ValueError, match="replace_cylinder_with_capsule"):
        NativeSetup(cfg, sim_params_for(cfg), model, terrain=ter, seed=0)
    cfg.asset.replace_cylinder_with_capsule = True
    s2 = NativeSetup(cfg, sim_params_for(cfg), model, terrain=ter, seed=0)
    assert s2.lattice_mesh_capsules is True and s2.terrain.mesh_type == abi.LG_MESH_TRIMESH
    # the biped's instance has no lattice-mesh path
    from extended_legged_gym_amd.envs.cassie.cassie_config import CassieRoughCfg
    cc = CassieRoughCfg()
    cc.env.num_envs = 4
    cc.terrain.mesh_type = "plane"
    cc.terrain.lattice_mesh_capsules = True
    with pytest.raises(ValueError, match="Cassie"):
        NativeSetup(cc, sim_params_for(cc), load_robot_model(cc.asset), seed=0)
    # declared in the C header, exported by the product library's symbol list (build() resolves every one of them)
    hdr = open(os.path.join(ROOT, "include", "lgstep.h")).read()
    assert "int lg_set_lattice_capsules(lg_ctx* ctx, int32_t on);" in hdr
    assert "lg_set_lattice_capsules" in abi.PRODUCT_SYMBOLS
    so = os.path.join(ROOT, "extended_legged_gym_amd", "csrc", "liblgstep.so")
    if os.path.exists(so):
        import ctypes
        ctypes.CDLL(so).lg_set_lattice_capsules


# ------------------------------------------------------------------------------------------------------------------------------------ CPU: resource budget
PRE_EXISTING = os.path.join(ROOT, "tests", "golden", "physics_kernel_resources_main.json")


def _sgpr_counts(legs):
    """.sgpr_count of every kernel in the code object of csrc/lg_step<legs>.o when that object is current (test_kernel_resources._from_built_object's rule)."""
    from tests.abi_checks import CSRC, object_metadata
    from tests.test_kernel_resources import _from_built_object
    obj = os.path.join(CSRC, f"lg_step{legs}.o")
    if _from_built_object(obj) is None:
        return {}
    return {k: r["sgpr_count"] for k, r in object_metadata(obj).items() if "sgpr_count" in r}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
@pytest.mark.parametrize("legs", [4, 6])
def test_lattice_capsule_instances_fit_and_leave_the_others_alone(tmp_path, legs):
    """Every physics_kernel instance with FEAT bit 2 (SPEC & 16): no vector spills, scratch <= 64 B, one workgroup's LDS -- WAIVED for one instance, the
    quadruped's lattice + self-collision step (DESIGN s3), which is held to its grid-mesh twin's spill instead.  Every physics_kernel instance that
    existed before the feature reports the register / LDS numbers it had (tests/golden/physics_kernel_resources_main.json: the built code object's metadata
    of the parent commit)."""
    from tests.test_kernel_resources import _resources
    blocks = _resources(tmp_path, legs)
    for k, n_sgpr in _sgpr_counts(legs).items():        # (the built object's metadata; the compile fall-back of _resources reports them itself)
        if k in blocks:
            blocks[k]["SGPRs"] = n_sgpr
    pre = "_ZN3lg%d14physics_kernelI" % legs
    import re

    def spec(name):        # physics_kernel<MODE, TMESH, HELPERS, SPEC>: the last template argument
        m = re.match(r"_ZN3lg\d14physics_kernelILi(\d+)ELb([01])ELb([01])ELi(\d+)E", name)
        return None if m is None else (int(m.group(1)), m.group(2) == "1", m.group(3) == "1", int(m.group(4)))
    new = [k for k in blocks if k.startswith(pre) and spec(k) and spec(k)[3] & 16]
    want = 5 if legs == 4 else 3          # step +- self-collision, rollout tail +- self-collision (four legs only), lg_simulate's single-wave instance
    assert len(new) == want, sorted(k for k in blocks if k.startswith(pre))
    for k in new:
        r = blocks[k]
        assert spec(k)[1], k                                                   # triangle-mesh instances only
        assert r["LDS Size"] <= 160 * 1024, (k, r)
        if legs == 4 and spec(k)[:3] == (0, True, True) and spec(k)[3] == 16 + 8:
            # the quadruped's lattice + self-collision step: at the register file's edge like its grid-mesh counterpart <0,true,true,12> (which ships with
            # 4 VGPRs spilled, 80 B scratch); it may not spill more than that one
            grid = [g for g in blocks if g.startswith(pre) and spec(g) == (0, True, True, 12)]
            assert len(grid) == 1 and r["VGPRs Spill"] <= blocks[grid[0]]["VGPRs Spill"] and r["ScratchSize"] <= blocks[grid[0]]["ScratchSize"], (k, r)
        else:
            assert r["VGPRs Spill"] == 0 and r["ScratchSize"] <= 64, (k, r)
    ref = json.load(open(PRE_EXISTING))[str(legs)]
    for k, want_r in ref.items():
        assert k in blocks, k
        for f in ("VGPRs", "AGPRs", "SGPRs", "LDS Size"):
            if f in want_r and f in blocks[k]:
                assert blocks[k][f] == want_r[f], (k, f, blocks[k][f], want_r[f])


# ------------------------------------------------------------------------------------------------------------------------------------------ GPU helpers
def obj_setup(tmp_path, n, verts_world, tris, name, caps=False, gravity=None, control="T"):
    """anymal_c_rough's robot (as stairs_setup) on the triangle mesh `verts_world` written to an OBJ file and loaded back through TerrainObj -- a LATTICE mesh
    (contact queries by lattice cell), not a grid mesh.  TerrainObj centres the mesh in xy: world = file - centre.  Returns (setup, offset) with
    offset = the xy shift from `verts_world` to where the mesh stands."""
    from extended_legged_gym_amd.envs.base.native_config import NativeSetup
    from extended_legged_gym_amd.utils.obj_io import save_obj
    from extended_legged_gym_amd.utils.terrain_obj import TerrainObj
    from tests.helpers import ANYMAL_GAIT, sim_params_for
    cfg, _, _, model = stairs_setup(n)
    path = os.path.join(str(tmp_path), name + ".obj")
    save_obj(path, verts_world, tris)
    t = cfg.terrain
    # (2 x 2 tiles: TerrainObj's placeholder height grid must not have the mesh's vertex count, or NativeSetup takes the mesh for a procedural grid mesh)
    t.mesh_type, t.use_terrain_obj, t.terrain_file, t.curriculum, t.num_rows, t.num_cols = "trimesh", True, path, False, 2, 2
    t.lattice_mesh_capsules = caps
    if gravity is not None:
        cfg.sim.gravity = list(gravity)
    cfg.control.control_type = control
    tobj = TerrainObj(t)
    s = NativeSetup(cfg, sim_params_for(cfg), model, terrain=tobj, seed=0, gait=ANYMAL_GAIT)
    assert s.terrain.mesh_type == abi.LG_MESH_TRIMESH and not bool(s.terrain.grid_vertices)
    v = np.asarray(verts_world, np.float64)
    off = np.asarray(s.collision_vertices, np.float64)[:, :2].mean(0) - v[:, :2].mean(0)
    return s, model, off


def make_core(s, root, dof, caps):
    import torch
    from extended_legged_gym_amd.native import NativeCore
    s.lattice_mesh_capsules = bool(caps)
    core = NativeCore(s, "cuda:0")
    core.t["friction_coeffs"].fill_(1.0)
    core.t["root_states"].copy_(torch.from_numpy(root))
    core.t["dof_state"].copy_(torch.from_numpy(dof.reshape(tuple(core.t["dof_state"].shape))))
    core.t["torques"].zero_()
    return core


def even_stairs_setup(n):
    """stairs_setup's staircase with a flat strip two cells wide along its y = 0 edge.  The slope correction moves the whole row of vertices at every riser onto
    the neighbouring x line, so the plain staircase leaves every third x line of its lattice without a vertex: uneven boundaries, no contact lattice (tree-walked,
    like any mesh that is not a lattice).  In the strip nothing moves and every line keeps its vertices.  The robots stand 1.7 m and more from the strip."""
    from extended_legged_gym_amd.envs.base.native_config import NativeSetup
    from extended_legged_gym_amd.utils import terrain_utils
    from tests.helpers import ANYMAL_GAIT, sim_params_for
    cfg, ter, _, model = stairs_setup(n)
    t = cfg.terrain
    ter.height_field_raw[:, :2] = 0
    ter.heightsamples = ter.height_field_raw
    ter.vertices, ter.triangles = terrain_utils.convert_heightfield_to_trimesh(ter.height_field_raw, t.horizontal_scale, t.vertical_scale, t.slope_treshold)
    grid = NativeSetup(cfg, sim_params_for(cfg), model, terrain=ter, seed=0, gait=ANYMAL_GAIT)
    assert grid.terrain.mesh_type == abi.LG_MESH_TRIMESH and bool(grid.terrain.grid_vertices)
    return cfg, ter, grid, model


def stairs_obj(tmp_path, n, caps=False):
    """The staircase (even_stairs_setup) as a lattice OBJ mesh; the grid setup, its model and the xy offset between the two."""
    cfg, ter, grid, model = even_stairs_setup(n)
    v = np.asarray(ter.vertices, np.float64) - np.array([cfg.terrain.border_size, cfg.terrain.border_size, 0.0])     # where the grid mesh stands
    s, model, off = obj_setup(tmp_path, n, v, ter.triangles, "stairs", caps)
    return grid, s, model, off


def shifted(root, geom, off):
    r = root.copy()
    r[:, 0] += off[0]; r[:, 1] += off[1]
    body, pos, sl, xw, zt = geom
    return r, (body, pos, sl, xw + off[0], zt)


def loaded(core, n, bodies):
    cf = core.t["contact_forces"].cpu().numpy().reshape(n, -1, 3)
    return np.linalg.norm(cf[np.arange(n), bodies], axis=1) > 1.0


# --------------------------------------------------------------------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
def test_lattice_segment_holds_a_shank_on_a_nosing(tmp_path):
    """Known answer on the OBJ staircase: shanks lowered onto nosings between two of their spheres.  On: at least n / 10 of them are answered only by the
    segment in the first substep, the segments never take a contact away, and 16 substeps on they are held (clearance > -2 mm).  Off: a quarter of them
    are more than 5 mm in."""
    import torch
    n = 256
    grid, s, model, off = stairs_obj(tmp_path, n)
    root, dof, geom = stairs_states(grid, model, n, seed=3)
    root, geom = shifted(root, geom, off)
    first, last = {}, {}
    for caps in (1, 0):
        core = make_core(s, root, dof, caps)
        assert core.collision_mesh.contact_lattice != (0, 0)
        for it in range(16):
            core.simulate()
            if it == 0:
                first[caps] = loaded(core, n, geom[0])
        torch.cuda.synchronize()
        assert torch.isfinite(core.t["root_states"]).all()
        last[caps] = nosing_clearance(core.t["rigid_body_state"].cpu().numpy(), geom)
        core.close()
    only = first[1] & ~first[0]
    assert only.sum() >= n // 10 and not (first[0] & ~first[1]).any(), (int(only.sum()), int((first[0] & ~first[1]).sum()))
    assert last[1][only].min() > -2e-3, float(last[1][only].min())
    assert np.quantile(last[0][only], 0.25) < -5e-3, float(np.quantile(last[0][only], 0.25))


def ceiling_mesh(z_hi=1.0, z_lo=0.6, size=4.0, h=0.1, vs=0.005):
    """Two layers: a flat ground at 0 and a ceiling at z_hi for x < size / 2, z_lo beyond -- after the slope correction a vertical step in the ceiling whose
    lower edge (x_e, z_lo) runs along y.  Returns vertices, triangles, x_e."""
    from extended_legged_gym_amd.utils.terrain_confine import convert_2layer_heightfield_to_trimesh
    r = int(size / h) + 1
    g = np.zeros((r, r), np.int16)
    c = np.full((r, r), int(round(z_hi / vs)), np.int16)
    c[r // 2:, :] = int(round(z_lo / vs))
    v, tri = convert_2layer_heightfield_to_trimesh(g, c, h, vs, 0.75, enable_ceiling=True, global_noise=0.0)
    v = np.asarray(v, np.float64)
    lower = v[(v[:, 2] > 0.5 * (z_lo + 0)) & (np.abs(v[:, 2] - z_lo) < 1e-4)]
    return v, np.asarray(tri), float(lower[:, 0].min())


@pytest.mark.gpu
def test_lattice_segment_holds_a_shank_under_a_ceiling_edge(tmp_path):
    """Known answer under a CEILING: no gravity, every robot rising at 0.2 m/s with the middle of one shank segment just under the step edge of the ceiling
    (4 mm in to 6 mm clear).  On: the shanks only the segment answers are held (clearance > -2 mm after 16 substeps).  Off: they enter.  A sign rule that
    only works facing up (outside = above the edge) pulls them in instead."""
    import torch
    n = 256
    v, tri, xe = ceiling_mesh()
    s, model, off = obj_setup(tmp_path, n, v, tri, "ceiling", gravity=(0.0, 0.0, 0.0))
    _, _, grid, _ = stairs_setup(n)
    root, dof, (body, pos, sl, xw, zt) = stairs_states(grid, model, n, seed=4)
    # move each robot from its nosing to the ceiling's edge: the segment's middle R_SHANK + [-4, 6] mm below (x_e, z_lo), rising
    from oracle.oracle_lib import OracleEnv
    from tests.test_mesh_capsules import _quat_rot
    o = OracleEnv(grid)
    load_oracle(o, root, dof)
    o.refresh_rigid_body_state()
    rb = o.t["rigid_body_state"].reshape(n, -1, 13).copy()
    o.close()
    mid = rb[np.arange(n), body, :3] + _quat_rot(rb[np.arange(n), body, 3:7], pos + 0.5 * sl)
    rng = np.random.default_rng(5)
    zc, xe_w = 0.6, xe + off[0]
    root[:, 0] += xe_w - mid[:, 0]
    root[:, 1] += off[1]
    root[:, 2] += zc - R_SHANK - rng.uniform(-0.004, 0.006, n) - mid[:, 2]
    root[:, 9] = 0.2
    geom = (body, pos, sl, np.full(n, xe_w), np.full(n, zc))

    def clearance(rb):      # signed distance from the edge to the segment's axis (xz plane) minus the radius; negative: in the ceiling (above the edge)
        rb = np.asarray(rb).reshape(n, -1, 13)
        p, q = rb[np.arange(n), body, :3], rb[np.arange(n), body, 3:7]
        a, b = p + _quat_rot(q, pos), p + _quat_rot(q, pos + sl)
        dx, dz = b[:, 0] - a[:, 0], b[:, 2] - a[:, 2]
        t = np.clip(((xe_w - a[:, 0]) * dx + (zc - a[:, 2]) * dz) / (dx * dx + dz * dz), 0, 1)
        cx, cz = a[:, 0] + t * dx, a[:, 2] + t * dz
        d = np.hypot(cx - xe_w, cz - zc)
        return np.where(cz <= zc, d, -d) - R_SHANK
    first, last = {}, {}
    for caps in (1, 0):
        core = make_core(s, root, dof, caps)
        for it in range(16):
            core.simulate()
            if it == 0:
                first[caps] = loaded(core, n, body)
        torch.cuda.synchronize()
        assert torch.isfinite(core.t["root_states"]).all()
        last[caps] = clearance(core.t["rigid_body_state"].cpu().numpy())
        core.close()
    only = first[1] & ~first[0]
    assert only.sum() >= n // 10 and not (first[0] & ~first[1]).any(), (int(only.sum()), int((first[0] & ~first[1]).sum()))
    assert last[1][only].min() > -2e-3, float(last[1][only].min())
    assert np.quantile(last[0][only], 0.25) < -5e-3, float(np.quantile(last[0][only], 0.25))


@pytest.mark.gpu
def test_lattice_segments_agree_with_the_oracle_pinned_grid_path(tmp_path):
    """The same staircase and states as a GRID mesh (`contact_detect_mesh<true>`, pinned to the oracle by test_mesh_capsules.py) and as a lattice OBJ mesh with
    the switch on.  Among the shanks that either path answers with the segment (loaded with it, not without it), at least 95 % carry a contact force on both,
    and both hold them 16 substeps on.  Where they disagree: the grid rule takes the mesh's edge between vertices (L, j) and (L, j + 1) of the height grid's
    rows; after the slope correction a riser's vertices moved a cell, so the lattice line the ground track crosses first can be a different line of the
    lattice (the foot or the top of the riser instead of the nosing) -- same surface, another edge of it; those are the few percent allowed."""
    import torch
    from extended_legged_gym_amd.native import NativeCore
    n = 256
    grid, s, model, off = stairs_obj(tmp_path, n)
    root, dof, geom = stairs_states(grid, model, n, seed=2)
    root_o, geom_o = shifted(root, geom, off)

    def grid_core(mesh_caps):
        old = os.environ.get("LG_MESH_CAPS")
        os.environ["LG_MESH_CAPS"] = "1" if mesh_caps else "0"
        try:
            core = NativeCore(grid, "cuda:0")
        finally:
            if old is None:
                del os.environ["LG_MESH_CAPS"]
            else:
                os.environ["LG_MESH_CAPS"] = old
        core.t["friction_coeffs"].fill_(1.0)
        core.t["root_states"].copy_(torch.from_numpy(root))
        core.t["dof_state"].copy_(torch.from_numpy(dof.reshape(tuple(core.t["dof_state"].shape))))
        core.t["torques"].zero_()
        return core
    cores = {"grid": grid_core(True), "grid0": grid_core(False), "lat": make_core(s, root_o, dof, 1), "lat0": make_core(s, root_o, dof, 0)}
    for c in cores.values():
        c.simulate()
    torch.cuda.synchronize()
    ld = {k: loaded(c, n, geom[0]) for k, c in cores.items()}
    seg = (ld["grid"] & ~ld["grid0"]) | (ld["lat"] & ~ld["lat0"])
    both = ld["grid"] & ld["lat"]
    assert seg.sum() >= n // 10 and both[seg].mean() >= 0.95, (int(seg.sum()), float(both[seg].mean()))
    for _ in range(15):
        for c in cores.values():
            c.simulate()
    torch.cuda.synchronize()
    cg = nosing_clearance(cores["grid"].t["rigid_body_state"].cpu().numpy(), geom)
    cl = nosing_clearance(cores["lat"].t["rigid_body_state"].cpu().numpy(), geom_o)
    assert cg[seg & both].min() > -2e-3 and cl[seg & both].min() > -2e-3, (float(cg[seg & both].min()), float(cl[seg & both].min()))
    for c in cores.values():
        c.close()


@pytest.mark.gpu
def test_no_candidate_no_change(tmp_path):
    """A flat lattice mesh, robots standing and stepping on it with small PD actions, shanks never near an edge: 50 policy steps with the switch on and off give
    bit-identical root / dof / contact-force / observation tensors."""
    import torch
    n = 64
    s, model, off = flat_obj(tmp_path, n, control="P")      # (PD about the default pose: the robots stand and step)
    rng = np.random.default_rng(0)
    root = np.zeros((n, 13), np.float32)
    root[:, 0], root[:, 1], root[:, 2], root[:, 6] = rng.uniform(1.0, 4.0, n) + off[0], rng.uniform(1.0, 4.0, n) + off[1], 0.62, 1.0
    dof = np.zeros((n, 12, 2), np.float32)
    dof[:, :, 0] = np.asarray(s.default_dof_pos)
    g = torch.Generator().manual_seed(0)
    acts = [(0.2 * torch.randn(n, 12, generator=g)).cuda() for _ in range(50)]
    out = {}
    for caps in (1, 0):
        core = make_core(s, root, dof, caps)
        for a in acts:
            core.step(a)
        torch.cuda.synchronize()
        out[caps] = {k: core.t[k].cpu().clone() for k in ("root_states", "dof_state", "contact_forces", "obs_buf")}
        core.close()
    assert torch.isfinite(out[1]["root_states"]).all()
    for k in out[1]:
        assert torch.equal(out[1][k], out[0][k]), k


def flat_obj(tmp_path, n, control="T"):
    """A flat 6 m x 6 m lattice mesh (the staircase's triangulation of a zero height grid) at the staircase's place: every lattice line is an edge, none a crease."""
    from extended_legged_gym_amd.utils import terrain_utils
    size, h = 6.0, 0.1
    r = int(size / h) + 1
    v, tri = terrain_utils.convert_heightfield_to_trimesh(np.zeros((r, r), np.int16), h, 0.005, 0.75)
    v = np.asarray(v, np.float64) - np.array([1.0, 1.0, 0.0])
    return obj_setup(tmp_path, n, v, tri, "flat", control=control)


@pytest.mark.gpu
def test_shanks_lying_on_flat_ground_change_nothing(tmp_path):
    """Shanks lowered onto FLAT lattice ground (segment middle 4 mm in to 6 mm clear, sinking): the segments reach the lattice lines' edges in every substep,
    and on a plane a segment is never deeper than its end spheres -- the edges there are no creases (coplanar owners), so 16 substeps with the switch on and
    off are bit-identical."""
    import torch
    n = 256
    s, model, off = flat_obj(tmp_path, n)
    _, _, grid, _ = even_stairs_setup(n)
    root, dof, geom = stairs_states(grid, model, n, seed=7, rise=0.0)            # (rise 0: the "nosings" are lattice lines of the flat ground)
    root, geom = shifted(root, geom, off)
    out, first = {}, {}
    for caps in (1, 0):
        core = make_core(s, root, dof, caps)
        for it in range(16):
            core.simulate()
            if it == 0:
                first[caps] = loaded(core, n, geom[0])
        torch.cuda.synchronize()
        out[caps] = {k: core.t[k].cpu().clone() for k in ("root_states", "dof_state", "contact_forces", "rigid_body_state")}
        core.close()
    assert first[0].sum() >= n // 4, int(first[0].sum())                      # the shanks do touch the ground
    assert torch.isfinite(out[1]["root_states"]).all()
    for k in out[1]:
        assert torch.equal(out[1][k], out[0][k]), k


@pytest.mark.gpu
def test_one_edge_near_shank_per_wave_matches_the_dense_run(tmp_path):
    """What one env's shank meets may not depend on the other envs of its wave (16 envs per wave): the staircase's states with only every 16th env on its
    nosing, the others lifted 1.5 m clear of everything.  The nosings run along y and are constant-x lattice edges, which no face of the slope-corrected
    triangulation lists FIRST -- a face loop that skipped its vertex rotation whenever no lane of the wave had a candidate missed them.  Those envs match the
    run in which every env is on a nosing, and the shanks only the segment answers are held when alone."""
    import torch
    n = 1024
    grid, s, model, off = stairs_obj(tmp_path, n)
    root, dof, geom = stairs_states(grid, model, n, seed=3)
    root, geom = shifted(root, geom, off)
    near = np.arange(n) % 16 == 0
    sparse = root.copy()
    sparse[~near, 2] += 1.5
    first, state = {}, {}
    for name, caps, r in (("dense", 1, root), ("off", 0, root), ("sparse", 1, sparse)):
        core = make_core(s, r, dof, caps)
        for it in range(16):
            core.simulate()
            if it == 0:
                first[name] = loaded(core, n, geom[0])
                state[name + "1"] = {k: core.t[k].cpu().numpy().reshape(n, -1).copy() for k in ("root_states", "dof_state", "contact_forces")}
        torch.cuda.synchronize()
        state[name] = {k: core.t[k].cpu().numpy().reshape(n, -1).copy() for k in ("root_states", "dof_state", "contact_forces", "rigid_body_state")}
        core.close()
    assert (first["sparse"][near] == first["dense"][near]).all()
    for k in ("root_states", "dof_state", "contact_forces"):
        for tag in ("1", ""):
            a, b = state["sparse" + tag][k][near], state["dense" + tag][k][near]
            assert np.abs(a - b).max() <= 1e-5 * max(1.0, float(np.abs(b).max())), (k, tag, float(np.abs(a - b).max()))
    only = near & first["dense"] & ~first["off"]
    assert only.sum() >= 3, int(only.sum())
    assert nosing_clearance(state["sparse"]["rigid_body_state"], geom)[only].min() > -2e-3


@pytest.mark.gpu
def test_rollout_tail_carries_the_lattice_segments(tmp_path):
    """A main-rollout layout on the OBJ staircase, shanks on nosings: the fused ROLLOUT tail's lattice-segment instance (`lg_step_subset`, rollout_mode 1)
    holds the shanks the standalone step of the same envs holds (`lg_step_subset_physics`: the step instance, no tail), and its physics state matches that
    step's at the bars of tests/test_hip_vs_oracle.py."""
    import torch
    from tests.test_hip_vs_oracle import compare
    M, R = 32, 3
    n = M * (1 + R)
    grid, s, model, off = stairs_obj(tmp_path, n)
    root, dof, geom = stairs_states(grid, model, n, seed=6)
    root, geom = shifted(root, geom, off)
    roll = np.array([e for e in range(n) if e % (1 + R)], dtype=np.int32)
    rng = np.random.default_rng(0)
    a = (0.5 * rng.normal(size=(len(roll), 12))).astype(np.float32)
    res = {}
    for name, caps, mode in (("tail", 1, 1), ("plain", 1, None), ("off", 0, 1)):
        core = make_core(s, root, dof, caps)
        if mode is None:           # the standalone physics of the same envs (lg_step_subset_physics: the step instance, no tail)
            core.step_subset_physics(torch.from_numpy(a).cuda(), torch.from_numpy(roll).cuda())
        else:
            core.step_subset(torch.from_numpy(a).cuda(), torch.from_numpy(roll).cuda(), mode)
        torch.cuda.synchronize()
        res[name] = core
    ids = roll

    class Ref:                     # the standalone step's tensors, as compare() reads an oracle's (rollout envs are never reset by the tail)
        t = {k: res["plain"].t[k].cpu().numpy() for k in ("root_states", "dof_state", "contact_forces")}
    rows = np.zeros(n, bool); rows[ids] = True
    compare(res["tail"], Ref, ["root_states", "dof_state", "contact_forces"], bars="step_tgs_mesh", rows=rows, tag="rollout_step/lattice_capsules")
    on, plain = loaded(res["tail"], n, geom[0])[ids], loaded(res["plain"], n, geom[0])[ids]
    assert (on == plain).mean() >= 0.97
    assert on.sum() >= len(ids) // 10, int(on.sum())              # the shanks carry load; holding them is the standalone step's, which the known answers pin
    for c in res.values():
        c.close()


@pytest.mark.gpu
def test_config3_soak_with_lattice_segments(tmp_path, monkeypatch):
    """Config 3 (A1 on the confined barrier + timber-pile OBJ mesh) with the switch on: 200 steps of N(0, 1) actions, every value finite, no env below the mesh
    (the check of tests/test_hip_config3.py::test_a1_on_confined_obj_mesh_never_falls_through)."""
    import torch
    from extended_legged_gym_amd.envs.a1.a1_config import A1RoughCfg
    from tests.test_hip_config3 import make_env
    monkeypatch.setattr(A1RoughCfg.terrain, "lattice_mesh_capsules", True, raising=False)
    n, steps = 512, 200
    env, cfg, (v, tri) = make_env(tmp_path, n, rows=2, cols=2)
    assert env.setup.lattice_mesh_capsules and env.core.collision_mesh.contact_lattice != (0, 0)
    zmin = float(v[:, 2].min())
    env.reset()
    g = torch.Generator().manual_seed(1)
    z_low = 1e9
    for _ in range(steps):
        env.step(torch.randn(n, 12, generator=g).cuda())
        z_low = min(z_low, float(env.root_states[:, 2].min()))
    torch.cuda.synchronize()
    assert torch.isfinite(env.root_states).all() and torch.isfinite(env.obs_buf).all() and torch.isfinite(env.dof_state).all()
    assert z_low > zmin - 1.0, z_low


@pytest.mark.gpu
def test_hexapod_on_a_confined_mesh_with_lattice_segments():
    """The six-legged instance carries the feature too: `elspider_air_rough_raycast` on its confined two-layer lattice mesh with the switch on, 20 steps of
    small random actions: finite, above the ground."""
    import torch
    from tests.test_env_api import make
    env = make("elspider_air_rough_raycast", 64, **{"terrain.num_rows": 2, "terrain.num_cols": 3, "terrain.confined_terrain_proportions": [0.0, 0.2, 0.4, 0.4],
                                                   "terrain.lattice_mesh_capsules": True})
    assert env.setup.lattice_mesh_capsules and env.setup.num_legs == 6 and env.core.collision_mesh.contact_lattice != (0, 0)
    assert np.abs(np.asarray(env.setup.model_dict["cp_slide"])).max() > 0     # the hexapod's capsules carry segments
    env.reset()
    g = torch.Generator().manual_seed(4)
    for _ in range(20):
        obs, _, rew, _, _ = env.step(0.2 * torch.randn(64, 18, generator=g).cuda())
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all() and torch.isfinite(env.root_states).all()
    assert float(env.root_states[:, 2].min()) > 0.05
    env.core.close()
