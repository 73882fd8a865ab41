"""Cassie (the 2 x 6 chain instance, `csrc/lg_chain.h`) on triangle meshes that are not grid meshes: OBJ and confined two-layer terrains.  Their contact
queries walk the BVH (`closest_point`) in the `physics_kernel_chain_bvh` instances.  Pinned against the oracle's brute-force scan, a known answer under a
ceiling, the helper waves against the single-wave launch, the grid mesh under `LG_GRID_MESH=0` against its grid path, the registered task on
`confined_trimesh`, and the compiler's resource report."""
import os

import numpy as np
import pytest

from tests.helpers import sim_params_for
from tests.test_kernel_resources import HIPCC, _resources

# timber piles, gaps, columns: a standing Cassie (pelvis ~1 m) fits under their ceilings; tunnels and barriers leave 0.4-0.9 m
PROPORTIONS = [0.0, 0.0, 0.4, 0.3, 0.3, 0.0]


def confined_cassie(n, seed):
    """Cassie on a small confined two-layer mesh (TerrainConfined: a lattice mesh, 0.2 m cells, 2 x 3 tiles of 4 m)."""
    from extended_legged_gym_amd.envs.base.native_config import NativeSetup, load_robot_model
    from extended_legged_gym_amd.envs.cassie.cassie_config import CassieRoughCfg
    from extended_legged_gym_amd.utils.terrain_confine import TerrainConfined
    cfg = CassieRoughCfg()
    cfg.env.num_envs = n
    t = cfg.terrain
    t.mesh_type = "confined_trimesh"
    t.num_rows, t.num_cols, t.border_size = 2, 3, 1.0
    t.terrain_length = t.terrain_width = 4.0
    t.horizontal_scale = 0.2
    t.max_init_terrain_level = 1
    t.confined_terrain_proportions = PROPORTIONS
    np.random.seed(seed)
    terrain = TerrainConfined(t, n)
    model = load_robot_model(cfg.asset)
    return cfg, NativeSetup(cfg, sim_params_for(cfg), model, terrain=terrain, seed=seed), terrain


def _core(s, monkeypatch, **env):
    from extended_legged_gym_amd.native import NativeCore
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    core = NativeCore(s, "cuda:0")
    for k in env:
        monkeypatch.delenv(k)
    return core


def _init_oracle(o, terrain, n, seed):
    rng = np.random.default_rng(seed)
    o.t["friction_coeffs"][:] = rng.uniform(0.5, 1.25, n)
    lv = rng.integers(0, 2, n); ty = np.floor(np.arange(n) / (n / 3)).astype(np.int64)
    o.t["terrain_levels"][:] = lv; o.t["terrain_types"][:] = ty
    o.t["env_origins"][:] = terrain.env_origins[lv, ty]
    o.reset_idx(np.arange(n))
    return rng


@pytest.mark.gpu
def test_confined_mesh_matches_the_oracle(monkeypatch):
    """`lg_compute_torques` + `lg_simulate` (bars "substep") and whole policy steps (step_bars) from states the oracle ran into.  The chain instance refused this
    terrain at construction before."""
    import torch
    from oracle.oracle_lib import OracleEnv
    from tests.test_hip_vs_oracle import COPY, STATE, compare, step_bars
    n = 128
    cfg, s, terrain = confined_cassie(n, 21)
    o = OracleEnv(s)
    core = _core(s, monkeypatch)
    assert not s.terrain.grid_vertices
    rng = _init_oracle(o, terrain, n, 11)
    loaded = 0
    for it in range(30):
        act = (0.5 * rng.normal(size=(n, 12))).astype(np.float32)
        if it % 5 == 4:
            for name in COPY:
                core.t[name].copy_(torch.from_numpy(o.t[name].copy()))
            keep = {k: o.t[k].copy() for k in COPY}
            o.compute_torques(act); o.simulate()
            core.compute_torques(torch.from_numpy(act).cuda()); core.simulate()
            compare(core, o, ["root_states", "dof_state", "rigid_body_state", "contact_forces", "torques"], bars="substep", tag="biped_substep/confined")
            loaded += int((np.abs(o.t["contact_forces"]).reshape(n, -1).max(axis=1) > 1.0).sum())
            for k in COPY:
                o.t[k][...] = keep[k]
                core.t[k].copy_(torch.from_numpy(keep[k]))
            o.step(act); core.step(torch.from_numpy(act).cuda())
            compare(core, o, STATE, bars=step_bars(s), tag="biped_step/confined")
            ra, rb = core.t["reset_buf"].cpu().numpy(), o.t["reset_buf"]
            assert (ra != rb).mean() <= 0.02
        else:
            o.step(act)
    assert loaded > n
    core.close(); o.close()


# a 6 m x 6 m floor at z = -0.2 and a 2 m x 2 m ceiling slab (z 0.95 .. 1.05) in its middle, lower than a standing Cassie's pelvis sphere reaches (~1.05 m)
ROOM_OBJ = """# room: floor and ceiling slab
v -3 -3 -0.2
v 3 -3 -0.2
v 3 3 -0.2
v -3 3 -0.2
v -1 -1 0.95
v 1 -1 0.95
v 1 1 0.95
v -1 1 0.95
v -1 -1 1.05
v 1 -1 1.05
v 1 1 1.05
v -1 1 1.05
f 1 2 3
f 1 3 4
f 5 7 6
f 5 8 7
f 9 10 11
f 9 11 12
f 5 6 10
f 5 10 9
f 6 7 11
f 6 11 10
f 7 8 12
f 7 12 11
f 8 5 9
f 8 9 12
"""


@pytest.mark.gpu
def test_ceiling_pushes_the_pelvis_down(tmp_path, monkeypatch):
    """Known answer: the pelvis sphere (radius 0.25 about the base origin) 3 cm into the underside of a ceiling slab.  After one `lg_simulate` the base's
    contact force points down, and it is the oracle's."""
    import torch
    from extended_legged_gym_amd import abi
    from extended_legged_gym_amd.envs.base.native_config import NativeSetup, load_robot_model
    from extended_legged_gym_amd.envs.cassie.cassie_config import CassieRoughCfg
    from extended_legged_gym_amd.utils.obj_io import load_obj
    from oracle.oracle_lib import OracleEnv
    from tests.test_hip_vs_oracle import compare
    from tests.test_oracle_physics import MeshFixtureTerrain, _mesh_cfg
    (tmp_path / "room.obj").write_text(ROOM_OBJ)
    v, tri = load_obj(str(tmp_path / "room.obj"))
    ter = MeshFixtureTerrain(v, tri, np.zeros((4, 4), np.int16), np.zeros((1, 1, 3), np.float32), 5.0)
    n = 16
    cfg = CassieRoughCfg()
    cfg.env.num_envs, cfg.env.num_observations = n, 48
    _mesh_cfg(cfg)
    s = NativeSetup(cfg, sim_params_for(cfg), load_robot_model(cfg.asset), terrain=ter, seed=3)
    assert s.terrain.mesh_type == abi.LG_MESH_TRIMESH and not s.terrain.grid_vertices
    o = OracleEnv(s)
    core = _core(s, monkeypatch)
    rng = np.random.default_rng(4)
    root = np.zeros((n, 13), np.float32)
    root[:, 0:2] = rng.uniform(-0.6, 0.6, size=(n, 2))
    root[:, 2] = 0.95 - 0.25 + 0.03                                   # the pelvis sphere's top 3 cm above the slab's underside; toes ~14 cm above the floor
    root[:, 6] = 1.0
    dof = np.zeros((n, 12, 2), np.float32)
    dof[:, :, 0] = s.default_dof_pos
    o.t["root_states"][:] = root; o.t["dof_state"][:] = dof
    o.t["friction_coeffs"][:] = 1.0; o.t["torques"][:] = 0.0
    o.refresh_rigid_body_state()
    core.t["root_states"].copy_(torch.from_numpy(root)); core.t["dof_state"].copy_(torch.from_numpy(dof))
    core.t["friction_coeffs"].fill_(1.0); core.t["torques"].zero_()
    o.simulate(); core.simulate()
    cf = core.t["contact_forces"].cpu().numpy().reshape(n, -1, 3)
    assert (cf[:, 0, 2] < -1.0).all() and (o.t["contact_forces"].reshape(n, -1, 3)[:, 0, 2] < -1.0).all(), cf[:, 0]
    compare(core, o, ["root_states", "dof_state", "rigid_body_state", "contact_forces"], bars="substep", tag="ceiling")
    np.testing.assert_allclose(cf[:, 0], o.t["contact_forces"].reshape(n, -1, 3)[:, 0], rtol=2e-3, atol=0.05)
    core.close(); o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,epb", [(45, None), (70, None), (70, "32")])
def test_helper_wave_detection_equals_the_single_wave_launch(n, epb, monkeypatch):
    """The tree-walk instance with its detection on three helper waves against the 64-thread launch (`LG_SPLIT=0`): every byte the library owns,
    60 steps with falls and resets, ragged env counts; mirrored halves up to 16 envs per workgroup, every lane its own (env, leg) under `LG_CHAIN_EPB=32`."""
    import torch
    if epb:
        monkeypatch.setenv("LG_CHAIN_EPB", epb)

    def build(split):
        cfg, s, terrain = confined_cassie(n, 3)
        s.cfg.episode_length_s = 0.6
        core = _core(s, monkeypatch, LG_SPLIT="1" if split else "0")
        rng = np.random.default_rng(1)
        lv = rng.integers(0, 2, n); ty = np.floor(np.arange(n) / (n / 3)).astype(np.int64)
        core.t["terrain_levels"].copy_(torch.from_numpy(lv)); core.t["terrain_types"].copy_(torch.from_numpy(ty))
        core.t["env_origins"].copy_(torch.from_numpy(terrain.env_origins[lv, ty].astype(np.float32)))
        core.reset_idx(torch.arange(n, device="cuda"))
        return core

    helped, inline = build(True), build(False)
    g = torch.Generator().manual_seed(4)
    resets = 0
    for it in range(60):
        a = (0.8 * torch.randn(n, 12, generator=g)).cuda()
        helped.step(a); inline.step(a)
        torch.cuda.synchronize()
        for name in helped.t:
            assert torch.equal(helped.t[name], inline.t[name]), (it, name)
        resets += int(helped.t["reset_buf"].sum())
    assert torch.equal(helped.arena, inline.arena)
    assert resets > 0 and torch.isfinite(helped.t["obs_buf"]).all()
    helped.close(); inline.close()


@pytest.mark.gpu
def test_task_cassie_on_confined_trimesh():
    """Task `cassie` through `task_registry.make_env` on `mesh_type = 'confined_trimesh'` (the chain instance refused it at construction before): 300 steps of
    random actions, everything finite, resets happen, no base below the mesh."""
    import torch
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.utils.helpers import get_args
    cfg, _ = task_registry.get_cfgs("cassie")
    cfg.env.num_envs = 256
    t = cfg.terrain
    t.mesh_type = "confined_trimesh"
    t.num_rows, t.num_cols, t.max_init_terrain_level = 3, 3, 2
    t.confined_terrain_proportions = PROPORTIONS
    env, _ = task_registry.make_env("cassie", args=get_args(["--headless", "--sim_device", "cuda:0"]), env_cfg=cfg)
    assert not env.setup.terrain.grid_vertices
    zmin = float(env.setup.collision_vertices[:, 2].min())
    env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    resets, z_low = 0, np.inf
    for _ in range(300):
        obs, _, rew, dones, _ = env.step(0.3 * torch.randn(256, 12, device="cuda:0", generator=g))
        resets += int(dones.sum())
        z_low = min(z_low, float(env.root_states[:, 2].min()))
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all() and torch.isfinite(env.root_states).all()
    assert resets > 0 and z_low > zmin - 1.0, (resets, z_low, zmin)
    env.core.close()


@pytest.mark.gpu
def test_grid_mesh_without_its_cells_agrees_with_the_grid_path(monkeypatch):
    """`LG_GRID_MESH=0` on the registered task's grid mesh: the sphere queries leave the grid cells for the tree-walk instance (the capsule segments
    against the mesh's own edges stay: they key on TerrainView::SEG4) and agree with the default path to the bars tests/test_mesh_capsules.py holds the
    quadruped's tree walk to."""
    import torch
    from oracle.oracle_lib import OracleEnv
    from tests.test_cassie import cassie_setup
    from tests.test_hip_vs_oracle import COPY

    def small_mesh(cfg):
        cfg.terrain.mesh_type = "trimesh"
        cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.border_size = 2, 2, 1
        cfg.terrain.terrain_length = cfg.terrain.terrain_width = 4.0
        cfg.terrain.max_init_terrain_level = 1
    n = 128
    _, s, terrain, _ = cassie_setup(n, "rough", mutate=small_mesh)
    assert bool(s.terrain.grid_vertices)
    o = OracleEnv(s)
    rng = np.random.default_rng(5)
    o.t["friction_coeffs"][:] = rng.uniform(0.5, 1.25, n)
    lv, ty = rng.integers(0, 2, n), rng.integers(0, 2, n)
    o.t["terrain_levels"][:] = lv; o.t["terrain_types"][:] = ty
    o.t["env_origins"][:] = terrain.env_origins[lv, ty]
    o.reset_idx(np.arange(n))
    for _ in range(12):
        o.step((0.5 * rng.normal(size=(n, 12))).astype(np.float32))
    grid, other = _core(s, monkeypatch), _core(s, monkeypatch, LG_GRID_MESH="0")
    for c in (grid, other):
        for name in COPY:
            c.t[name].copy_(torch.from_numpy(o.t[name].copy()))
        c.t["torques"].zero_()
    for _ in range(4):
        grid.simulate(); other.simulate()
    torch.cuda.synchronize()
    assert float(grid.t["contact_forces"].view(n, -1, 3).norm(dim=2).max()) > 50.0
    for name in ("root_states", "dof_state", "contact_forces"):
        a, b = grid.t[name].cpu().numpy().reshape(n, -1), other.t[name].cpu().numpy().reshape(n, -1)
        err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
        assert np.quantile(err, 0.999) < 1e-3 and np.median(err) < 1e-6, (name, float(err.max()))
    grid.close(); other.close(); o.close()


# ------------------------------------------------------------------------------------------------------------ CPU: the compiler's report
# the lg2 instances that existed before the tree-walk ones, as the parent build reported them: unchanged
EXISTING = {
    "_ZN3lg220physics_kernel_chainILi0ELb1ELb1E": dict(VGPRs=403, spill=0, scratch=112, lds=94664),
    "_ZN3lg220physics_kernel_chainILi0ELb0ELb1E": dict(VGPRs=402, spill=0, scratch=112, lds=94664),
    "_ZN3lg220physics_kernel_chainILi0ELb1ELb0E": dict(VGPRs=458, spill=0, scratch=112, lds=88264),
    "_ZN3lg220physics_kernel_chainILi0ELb0ELb0E": dict(VGPRs=407, spill=0, scratch=112, lds=88264),
    "_ZN3lg220physics_kernel_chainILi1ELb1ELb0E": dict(VGPRs=438, spill=0, scratch=112, lds=88264),
    "_ZN3lg220physics_kernel_chainILi1ELb0ELb0E": dict(VGPRs=389, spill=0, scratch=112, lds=88264),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_tree_walk_instances_fit(tmp_path):
    """The three new lg2 instances (policy step with and without helper waves, lg_simulate): no vector spills, one workgroup's LDS.  The walk keeps its
    traversal stack (BVH_STACK keys and node indices) in private memory: scratch, bounded, pinned at the measured bytes per lane; on the helper-wave
    instance the compiler moves part of the stack to LDS."""
    blocks = _resources(tmp_path, 2)

    def one(prefix):
        key = [k for k in blocks if k.startswith(prefix)]
        assert len(key) == 1, (prefix, sorted(blocks))
        return blocks[key[0]]
    for prefix, want in EXISTING.items():
        r = one(prefix)
        assert (r["VGPRs"] + r["AGPRs"], r["VGPRs Spill"], r["ScratchSize"], r["LDS Size"]) == (want["VGPRs"], want["spill"], want["scratch"], want["lds"]), (prefix, r)
    scratch = {(0, 1): 336, (0, 0): 432, (1, 0): 432}                      # bytes per lane, as measured (the grid-mesh instances: 112)
    for mode, help_ in scratch:
        r = one(f"_ZN3lg224physics_kernel_chain_bvhILi{mode}ELb{help_}E")
        print(mode, help_, r)
        assert r["VGPRs Spill"] == 0 and r["LDS Size"] <= 160 * 1024 and r["ScratchSize"] == scratch[(mode, help_)], r
