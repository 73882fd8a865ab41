"""Shared scenarios of the physics known answers (no tests here): one float64 `momenta` / `com` for every topology, one numpy face over the CPU
oracle and the HIP library, and the builders of the free-flight and contact scenarios that `tests/test_oracle_physics.py`, `tests/test_cassie.py` and
`tests/test_elspider.py` run on the oracle -- here for any of the three robots and for either side (`tests/test_hip_physics_known_answers.py`).

PhysX is closed, so the physics has no recorded reference: what pins it are statements that need no reference at all -- free fall at g,
conserved spin, momentum and energy, a stance that carries the weight, the friction limit, the momentum theorem over a landing."""
import ctypes as C

import numpy as np

ROBOTS = ("anymal_c", "elspider_air", "cassie")
G = 9.81
SOLVERS = [("tgs", "pyramid"), ("tgs", "cone"), ("pgs", "cone")]
STATE = ["root_states", "dof_state", "rigid_body_state"]


# ------------------------------------------------------------------------------------------------ momenta
def quat_to_mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sym(I6):
    return np.array([[I6[0], I6[1], I6[2]], [I6[1], I6[3], I6[4]], [I6[2], I6[4], I6[5]]], np.float64)


def topology(model):
    """(legs, joints per leg, rigid bodies per leg) of a robot model dict."""
    nl = int(model.get("num_legs", len(model["link_mass"])))
    nj = int(model.get("num_joints_per_leg", len(model["link_mass"][0])))
    return nl, nj, nj + int(model["has_foot_body"])


def bodies(model, added_mass=0.0):
    """(rigid-body row, mass, centre of mass in the body frame, inertia about it in the body frame) of every body that has mass: the base -- with the payload
    `added_mass`, which scales its inertia as the step does (m0 / base_mass) -- and the `num_joints_per_leg` links of every leg (a foot body is a massless
    frame behind the last link: `has_foot_body`)."""
    nl, nj, per_leg = topology(model)
    m0 = float(model["base_mass"])
    out = [(0, m0 + added_mass, np.asarray(model["base_com"], np.float64), sym(model["base_inertia"]) * ((m0 + added_mass) / m0))]
    for l in range(nl):
        for j in range(nj):
            out.append((1 + l * per_leg + j, float(model["link_mass"][l][j]), np.asarray(model["link_com"][l][j], np.float64), sym(model["link_inertia"][l][j])))
    return out


def total_mass(model, added_mass=0.0):
    return sum(b[1] for b in bodies(model, added_mass))


def momenta(model, rb, added_mass=0.0):
    """(total mass, linear momentum, angular momentum about the world origin, kinetic energy) in float64 from one env's (num_bodies, 13) rigid_body_state."""
    rb = np.asarray(rb, np.float64).reshape(-1, 13)
    M, P, L, K = 0.0, np.zeros(3), np.zeros(3), 0.0
    for b, m, c_b, I_b in bodies(model, added_mass):
        s = rb[b]
        R = quat_to_mat(s[3:7])
        r = R @ c_b
        w = s[10:13]
        v = s[7:10] + np.cross(w, r)
        Iw = R @ I_b @ R.T
        M += m
        P += m * v
        L += np.cross(s[0:3] + r, m * v) + Iw @ w
        K += 0.5 * m * (v @ v) + 0.5 * (w @ Iw @ w)
    return M, P, L, K


def com(model, rb, added_mass=0.0):
    """Centre of mass in the world frame (float64)."""
    rb = np.asarray(rb, np.float64).reshape(-1, 13)
    c, M = np.zeros(3), 0.0
    for b, m, c_b, _ in bodies(model, added_mass):
        c += m * (rb[b, 0:3] + quat_to_mat(rb[b, 3:7]) @ c_b)
        M += m
    return c / M


def spin(model, rb, added_mass=0.0):
    """Angular momentum about the centre of mass: what free flight conserves whatever the joints do."""
    _, P, L, _ = momenta(model, rb, added_mass)
    return L - np.cross(com(model, rb, added_mass), P)


# ------------------------------------------------------------------------------------------------ one face over the oracle and the HIP library
class Sim:
    """The calls and the tensors the scenarios need, in numpy, over an `OracleEnv` (`side = "oracle"`) or a `NativeCore` (`side = "hip"`)."""
    WRITABLE = ("root_states", "dof_state", "torques", "friction_coeffs", "base_mass_added", "commands", "env_origins")

    def __init__(self, setup, side):
        self.setup, self.side = setup, side
        self.n, self.nd = int(setup.cfg.num_envs), int(setup.num_dof)
        if side == "oracle":
            from oracle.oracle_lib import OracleEnv
            self.env = OracleEnv(setup)
        else:
            from extended_legged_gym_amd.native import NativeCore
            self.env = NativeCore(setup, "cuda:0")
        self.set("friction_coeffs", 1.0)

    # -- tensors
    def get(self, name):
        """A copy of tensor `name`; the per-body tensors come back as (envs, bodies, width)."""
        t = self.env.t[name]
        if self.side == "hip":
            import torch
            torch.cuda.synchronize()
            t = t.detach().cpu().numpy()
        a = np.array(t, copy=True)
        if name == "rigid_body_state":
            a = a.reshape(self.n, -1, 13)
        if name == "contact_forces":
            a = a.reshape(self.n, -1, 3)
        return a

    def set(self, name, value):
        t = self.env.t[name]
        if self.side == "hip":
            import torch
            v = np.broadcast_to(np.asarray(value, dtype=np.float32), tuple(t.shape)).copy()
            t.copy_(torch.from_numpy(v))
        else:
            t[...] = value

    def _act(self, actions):
        a = np.ascontiguousarray(actions, dtype=np.float32).reshape(self.n, self.nd)
        if self.side == "hip":
            import torch
            return torch.from_numpy(a).cuda()
        return a

    # -- calls
    def refresh(self):
        """The rigid-body states of the root / joint states just written (the oracle's refresh; a teleport of every env on the device)."""
        if self.side == "hip":
            import torch
            self.env.set_state_indexed(torch.arange(self.n))
        else:
            self.env.refresh_rigid_body_state()

    def compute_torques(self, actions):
        self.env.compute_torques(self._act(actions))

    def simulate(self):
        self.env.simulate()

    def step_physics(self, actions):
        """The physics half of a policy step: clip the actions, `decimation` x (actuator + one sim.dt) -- `lg_step_physics`, ONE launch on the device."""
        if self.side == "hip":
            self.env.compute_torques_and_simulate(self._act(actions))
        else:
            a = self._act(actions)
            ids = np.arange(self.n, dtype=np.int32)
            assert self.env.L.lgo_step_subset_physics(self.env.ctx, a.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), self.n) == 0

    def step(self, actions):
        self.env.step(self._act(actions))

    def reset_idx(self, ids=None):
        ids = np.arange(self.n) if ids is None else np.asarray(ids)
        if self.side == "hip":
            import torch
            self.env.reset_idx(torch.from_numpy(ids.astype(np.int64)))
        else:
            self.env.reset_idx(ids)

    def close(self):
        self.env.close()


# ------------------------------------------------------------------------------------------------ scenario builders
class Scenario:
    """A robot's config, native set-up and model dict; `sim(side)` opens the oracle or the HIP library on it."""

    def __init__(self, robot, cfg, setup, model):
        self.robot, self.cfg, self.setup, self.model = robot, cfg, setup, model
        self.n, self.nd = int(cfg.env.num_envs), int(setup.num_dof)
        self.mass = total_mass(model)
        self.sim_dt = float(setup.cfg.sim_dt)
        self.decimation = int(setup.cfg.decimation)
        self.action_scale = float(cfg.control.action_scale)
        _, _, per_leg = topology(model)
        self.num_bodies = int(model["num_bodies"])

    def sim(self, side):
        return Sim(self.setup, side)

    def actions_for_torques(self, tq):
        """Actions that make `control_type = "T"` command the torques `tq` (torque = action * action_scale, then the torque limit)."""
        return (np.asarray(tq, np.float64) / self.action_scale).astype(np.float32)


def flat_grid_terrain(cells=120):
    """A height grid whose cells are all equal (z = 0): the plane's answers through the grid's contact path."""
    from tests.helpers import FixtureTerrain
    return FixtureTerrain(np.zeros((cells, cells), np.int16), np.zeros((1, 1, 3), np.float32), 8.0)


def scenario(robot, n, gravity=(0.0, 0.0, -G), control="P", solver=None, dt=None, free=False, grid=False, self_collisions=True):
    """The set-up code of the oracle's own known-answer tests (`test_oracle_physics.make`, `test_cassie.cassie_setup`, `test_elspider.hexapod_setup`) for
    `robot`, with gravity, control type, (solver, friction model) and sim.dt as options.  `free`: a free-flight scenario -- the URDF's joint-speed cap (a
    clamp that conserves nothing) and the self-collision pass are off, as in the oracle's conservation tests.  `grid`: a flat height grid in place of the plane."""
    from extended_legged_gym_amd.envs.base.native_config import NativeSetup
    from tests.helpers import ELSPIDER_GAIT, sim_params_for
    def mut(cfg):
        cfg.control.control_type = control
        cfg.control.use_actuator_network = False
        cfg.sim.gravity = list(gravity)
        cfg.noise.add_noise = False
        cfg.domain_rand.push_robots = False
        if dt is not None:
            cfg.sim.dt = dt
        if solver is not None:
            cfg.sim.physx.solver_type = {"pgs": 0, "tgs": 1}[solver[0]]
            cfg.sim.physx.friction_model = solver[1]
        if free or not self_collisions:
            cfg.asset.self_collisions = 1                       # (PhysX's filter mask: 1 = the robot's own shapes do not collide)

    if robot == "anymal_c":
        from tests.helpers import ANYMAL_GAIT
        from tests.test_oracle_physics import make
        cfg, setup, model, o = make(n=n, control=control, gravity=gravity, mutate=mut, speed_limit=not free, solver=solver)
        o.close()
        kw = dict(seed=3, gait=ANYMAL_GAIT)
    elif robot == "cassie":
        from tests.test_cassie import cassie_setup
        cfg, setup, _, model = cassie_setup(n, "flat", seed=3, mutate=mut, gravity=gravity, control=control)
        kw = dict(seed=3)
    elif robot == "elspider_air":
        from tests.test_elspider import hexapod_setup
        cfg, setup, _, model = hexapod_setup(n, "flat_pd", mutate=mut)
        kw = dict(seed=11, gait=ELSPIDER_GAIT, terminate_on_flip=True)
    else:
        raise KeyError(robot)
    if free or grid:                  # (the set-up functions build plane set-ups with the URDF's speed cap: the same cfg with the options, as tests/test_cassie.py does)
        terrain = None
        if free:
            model = dict(model, dof_vel_limit=[0.0] * len(model["dof_names"]))
        if grid:
            terrain = flat_grid_terrain()
            cfg.terrain.mesh_type, cfg.terrain.border_size = "heightfield", 6.0
            cfg.terrain.num_rows = cfg.terrain.num_cols = 1
            cfg.terrain.curriculum = False
            cfg.terrain.horizontal_scale, cfg.terrain.vertical_scale = 0.1, 0.005
        setup = NativeSetup(cfg, sim_params_for(cfg), model, terrain=terrain, **kw)
    return Scenario(robot, cfg, setup, model)


def tumbling_state(sc, seed=0):
    """The start of `test_free_fall_com_accelerates_at_g_and_conserves_angular_momentum` for any robot: high above the ground, random attitude, root twist
    N(0, 1), joints around their default pose (Cassie, whose default pose sits near its limits: inside them as in `tests/test_cassie.py`), joint speeds
    2 N(0, 1), internal joint torques 5 N(0, 1).  Returns (root_states, dof_state, torques)."""
    rng = np.random.default_rng(seed)
    n, nd = sc.n, sc.nd
    root = np.zeros((n, 13), np.float32)
    root[:, 2] = 30.0 if sc.robot == "cassie" else 50.0
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    root[:, 3:7] = q
    root[:, 7:13] = rng.normal(size=(n, 6))
    dof = np.zeros((n, nd, 2), np.float32)
    if sc.robot == "cassie":
        lo, hi = np.asarray(sc.model["dof_lower"]), np.asarray(sc.model["dof_upper"])
        dof[:, :, 0] = 0.5 * (lo + hi) + 0.1 * (hi - lo) * rng.uniform(-1, 1, size=(n, nd))
    else:
        dof[:, :, 0] = sc.setup.default_dof_pos + 0.3 * rng.normal(size=(n, nd))
    dof[:, :, 1] = 2.0 * rng.normal(size=(n, nd))
    tq = (5.0 * rng.normal(size=(n, nd))).astype(np.float32)
    return root, dof, tq


def drifting_state(sc, seed=1):
    """The start of `test_zero_gravity_conserves_momentum_and_energy_without_torques` (Cassie: of `test_free_space_conserves_momentum_and_energy_and_falls_at_g`):
    level, 30 m up, twist and joint speeds of 0.5 N(0, 1) (quadruped and hexapod: joint speeds N(0, 1)), no torques."""
    rng = np.random.default_rng(seed)
    n, nd = sc.n, sc.nd
    root = np.zeros((n, 13), np.float32)
    root[:, 2], root[:, 6] = 30.0, 1.0
    root[:, 7:13] = 0.5 * rng.normal(size=(n, 6))
    dof = np.zeros((n, nd, 2), np.float32)
    if sc.robot == "cassie":
        lo, hi = np.asarray(sc.model["dof_lower"]), np.asarray(sc.model["dof_upper"])
        dof[:, :, 0] = 0.5 * (lo + hi) + 0.1 * (hi - lo) * rng.uniform(-1, 1, size=(n, nd))
        dof[:, :, 1] = 0.5 * rng.normal(size=(n, nd))
    else:
        dof[:, :, 0] = sc.setup.default_dof_pos + 0.2 * rng.normal(size=(n, nd))
        dof[:, :, 1] = 1.0 * rng.normal(size=(n, nd))
    return root, dof, np.zeros((n, nd), np.float32)


def place(sim, root, dof):
    """Write a state and bring the rigid-body states up to date; returns them."""
    sim.set("root_states", root)
    sim.set("dof_state", dof)
    sim.refresh()
    return sim.get("rigid_body_state")


def advance(sim, sc, actions, substeps, path):
    """`substeps` x sim.dt under constant actions: `path = "simulate"` goes substep by substep (`compute_torques` + `simulate`), `"step_physics"` takes
    `decimation` of them per call.  Returns the largest |contact force| seen and the lowest body origin (free flight: 0 and far above the ground)."""
    fmax, zmin = 0.0, np.inf
    if path == "simulate":
        for _ in range(substeps):
            sim.compute_torques(actions)
            sim.simulate()
    else:
        assert substeps % sc.decimation == 0
        for _ in range(substeps // sc.decimation):
            sim.step_physics(actions)
    # (contact forces are the last substep's; a robot 30 m up that touched anything on the way would not be here: the lowest body says so)
    fmax = max(fmax, float(np.abs(sim.get("contact_forces")).max()))
    zmin = min(zmin, float(sim.get("rigid_body_state")[:, :, 2].min()))
    return fmax, zmin


def free_flight_errors(sc, rb0, rb1, T, gravity=(0.0, 0.0, -G)):
    """Per env, float64: lin = |dP / M - g T|, ang = |change of the spin about the COM| / max(1, |spin|); and the masses."""
    g = np.asarray(gravity, np.float64)
    lin, ang, mass = [], [], []
    for e in range(sc.n):
        M, P0, _, _ = momenta(sc.model, rb0[e])
        _, P1, _, _ = momenta(sc.model, rb1[e])
        s0, s1 = spin(sc.model, rb0[e]), spin(sc.model, rb1[e])
        lin.append(np.linalg.norm((P1 - P0) / M - g * T))
        ang.append(np.linalg.norm(s1 - s0) / max(1.0, np.linalg.norm(s0)))
        mass.append(M)
    return np.array(lin), np.array(ang), np.array(mass)


def conservation_errors(sc, rb0, rb1):
    """Per env, float64, zero gravity and no torques: |dP| / M, |dK| / K, |dL| / max(1, |L|)."""
    dp, dk, dl = [], [], []
    for e in range(sc.n):
        M, P0, L0, K0 = momenta(sc.model, rb0[e])
        _, P1, L1, K1 = momenta(sc.model, rb1[e])
        dp.append(np.abs(P1 - P0).max() / M)
        dk.append(abs(K1 - K0) / K0)
        dl.append(np.abs(L1 - L0).max() / max(1.0, np.linalg.norm(L0)))
    return np.array(dp), np.array(dk), np.array(dl)


def ulp_nudge(a, rng):
    """Every entry of a float32 array moved to a neighbouring float32, up or down at random."""
    a = np.asarray(a, np.float32)
    toward = np.where(rng.integers(0, 2, size=a.shape) == 1, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    return np.nextafter(a, toward)


def relative_error(a, b):
    """err = |a - b| / max(1, |b|), every entry, float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


N_FREE, SEED_FREE = 37, 0      # envs and seed of the free-flight comparisons (the oracle alone meets their bars with them: tests/test_physics_known_answers.py)


def free_run(sc, side, root, dof, actions, substeps, path):
    """Rigid-body states before and after `substeps` of free flight; nothing may touch anything on the way."""
    sim = sc.sim(side)
    rb0 = place(sim, root, dof)
    fmax, zmin = advance(sim, sc, actions, substeps, path)
    out = {name: sim.get(name) for name in STATE + ["torques"]}
    sim.close()
    assert fmax == 0.0, f"{side}: contact force {fmax} in free flight"
    assert zmin > 10.0, f"{side}: lowest body at {zmin} m"
    return rb0, out


def one_call(sc, side, root, dof, actions, path):
    return free_run(sc, side, root, dof, actions, 1 if path == "simulate" else sc.decimation, path)[1]


def parity_inputs(robot):
    sc = scenario(robot, N_FREE, control="T", free=True)
    root, dof, tq = tumbling_state(sc, SEED_FREE)
    return sc, root, dof, sc.actions_for_torques(tq)


def yardstick(robot, path):
    """The oracle's own response to fp32 rounding of its inputs: eight seeded re-runs with every entry of root_states, dof_state and the torques moved to a
    neighbouring float32; per tensor the largest err = |moved - baseline| / max(1, |baseline|).  Returns (baseline, y)."""
    sc, root, dof, act = parity_inputs(robot)
    base = one_call(sc, "oracle", root, dof, act, path)
    y = {name: 0.0 for name in STATE}
    for k in range(8):
        rng = np.random.default_rng(100 + k)
        moved = one_call(sc, "oracle", ulp_nudge(root, rng), ulp_nudge(dof, rng), ulp_nudge(act, rng), path)
        for name in STATE:
            y[name] = max(y[name], float(relative_error(moved[name], base[name]).max()))
    return base, y


def bars_of(y):
    # 16: the two sides share no operation order (dense Cholesky there, per-leg Schur complement here); 2e-6: the project's fp32 atol
    return {name: max(16.0 * v, 2e-6) for name, v in y.items()}


# ------------------------------------------------------------------------------------------------ contact scenarios
STANCE = {      # payload rows [kg], base-height band [m], band of the base twist: the oracle tests' own (tests/test_oracle_physics.py, tests/test_elspider.py)
    "anymal_c": dict(payload=[0.0, 4.0], steps=100, height=(0.35, 0.65), twist=0.05, rtol=0.03),
    # (feet 0.159 m below the base origin + the 2 cm foot sphere; the hexapod's oracle test states no twist band: under TGS its stance keeps a 0.14 rad/s tremor)
    "elspider_air": dict(payload=np.linspace(-5, 5, 8).tolist(), steps=100, height=(0.168, 0.188), twist=None, rtol=0.03),
}      # (no row for the biped: with zero actions it topples within a second, on the oracle as on the device -- a stance is no known answer for it)


def stance_start(sim, sc):
    """The oracle tests' way into a stance: the quadruped from its reset pose at rest, the hexapod set down level at 0.2 m in its default pose."""
    sim.set("base_mass_added", np.asarray(STANCE[sc.robot]["payload"], np.float32))
    if sc.robot == "elspider_air":
        root = np.zeros((sc.n, 13), np.float32); root[:, 6] = 1; root[:, 2] = 0.2
        dof = np.zeros((sc.n, sc.nd, 2), np.float32); dof[:, :, 0] = sc.setup.default_dof_pos
        place(sim, root, dof)
    else:
        sim.reset_idx()
        root = sim.get("root_states"); root[:, 7:13] = 0
        sim.set("root_states", root)
        sim.refresh()


def stance_run(sim, sc, steps=None):
    z = np.zeros((sc.n, sc.nd), np.float32)
    resets = np.zeros(sc.n, bool)
    for _ in range(STANCE[sc.robot]["steps"] if steps is None else steps):
        sim.step(z)
        resets |= sim.get("reset_buf").astype(bool)
    return resets


def stance_figures(sim, sc, resets):
    """What a static stance is judged by: the summed vertical contact force over the weight, base height, largest base twist, lowest foot, smallest foot load."""
    payload = np.asarray(STANCE[sc.robot]["payload"], np.float64)
    cf, root, rb = sim.get("contact_forces").astype(np.float64), sim.get("root_states"), sim.get("rigid_body_state")
    feet = list(sc.model["feet_indices"])
    return dict(fz_over_weight=(cf[:, :, 2].sum(1) / ((sc.mass + payload) * G)).tolist(), base_z=root[:, 2].tolist(),
                twist=float(np.abs(root[:, 7:13]).max()), foot_z=float(rb[:, feet, 2].min()), foot_fz=float(cf[:, feet, 2].min()),
                resets=int(resets.sum()))


def check_stance(fig, sc):
    S = STANCE[sc.robot]
    assert np.all(np.abs(np.asarray(fig["fz_over_weight"]) - 1.0) <= S["rtol"]), fig
    assert np.all(np.asarray(fig["base_z"]) > S["height"][0]) and np.all(np.asarray(fig["base_z"]) < S["height"][1]), fig
    assert S["twist"] is None or fig["twist"] < S["twist"], fig
    assert fig["foot_z"] > -0.005, fig                           # feet do not sink into the ground
    assert fig["foot_fz"] > 1.0, fig                             # the reference's stance threshold (rew_mixin.py:153)
    assert fig["resets"] == 0, fig


def friction_limit_run(sim, sc, solver, steps=60, seed=5):
    """`test_friction_limit_holds_on_every_contact_body`: random actions on robots of friction 0.2 .. 1.2; returns (worst excess of |f_t| over mu f_n, lowest f_n)."""
    mu_robot = np.linspace(0.2, 1.2, sc.n).astype(np.float32)
    sim.set("friction_coeffs", mu_robot)
    sim.reset_idx()
    rng = np.random.default_rng(seed)
    mu = 0.5 * (mu_robot.astype(np.float64) + 1.0)[:, None]
    worst, fn_min = -np.inf, np.inf
    for _ in range(steps):
        sim.step(rng.normal(size=(sc.n, sc.nd)).astype(np.float32))
        F = sim.get("contact_forces").astype(np.float64)
        fn = F[:, :, 2]
        ft = np.linalg.norm(F[:, :, :2], axis=2) if solver[1] == "cone" else np.abs(F[:, :, :2]).max(axis=2)
        worst, fn_min = max(worst, float(np.max(ft - mu * fn))), min(fn_min, float(fn.min()))
    return worst, fn_min


def sliding_run(sim, sc):
    """`test_sliding_friction_decelerates_at_mu_g`: a stiffly standing robot pushed to 3 m/s on combined mu 0.6; returns the deceleration over three policy steps."""
    sim.set("friction_coeffs", 0.2)
    sim.reset_idx()
    root = sim.get("root_states"); root[:, 7:13] = 0
    sim.set("root_states", root); sim.refresh()
    z = np.zeros((sc.n, sc.nd), np.float32)
    for _ in range(50):
        sim.step(z)
    root, dof = sim.get("root_states"), sim.get("dof_state")
    root[0, 7] = 3.0; dof[0, :, 1] = 0
    sim.set("root_states", root); sim.set("dof_state", dof); sim.refresh()
    v = []
    for _ in range(6):
        sim.step(z)
        v.append(float(sim.get("root_states")[0, 7]))
    return -(v[4] - v[1]) / (3 * sc.sim_dt * sc.decimation)


LANDING = {"anymal_c": 0.9, "elspider_air": 0.5, "cassie": 0.9}      # base height the limp robot is dropped from, default pose [m]


def landing_run(sim, sc, substeps=100, seed=2):
    """`test_contact_forces_account_for_the_momentum_of_a_landing` for any robot: dropped limp (zero torques) in its default pose with a small sideways speed, 100 x
    `simulate`.  Returns (momentum change per env, impulse of (contact forces - weight) per env, peak vertical contact force per env)."""
    n = sc.n
    rng = np.random.default_rng(seed)
    root = np.zeros((n, 13), np.float32); root[:, 6] = 1; root[:, 2] = LANDING[sc.robot]
    root[:, 7:9] = 0.3 * rng.normal(size=(n, 2))
    dof = np.zeros((n, sc.nd, 2), np.float32); dof[:, :, 0] = sc.setup.default_dof_pos
    rb0 = place(sim, root, dof)
    z = np.zeros((n, sc.nd), np.float32)
    impulse, peak = np.zeros((n, 3)), np.zeros(n)
    weight = np.array([0.0, 0.0, sc.mass * G])
    for _ in range(substeps):
        sim.compute_torques(z)
        sim.simulate()
        F = sim.get("contact_forces").astype(np.float64).sum(axis=1)
        impulse += (F - weight) * sc.sim_dt
        peak = np.maximum(peak, F[:, 2])
    rb1 = sim.get("rigid_body_state")
    dP = np.array([momenta(sc.model, rb1[e])[1] - momenta(sc.model, rb0[e])[1] for e in range(n)])
    return dP, impulse, peak


def check_landing(sc, dP, impulse, peak, substeps=100):
    assert (peak > 2 * sc.mass * G).all(), peak                                              # they did land
    np.testing.assert_allclose(dP, impulse, atol=0.02 * sc.mass * G * substeps * sc.sim_dt)    # 2 % of the weight's impulse over the run
