"""The HIP physics kernels held to the analytic known answers that pin the oracle (`tests/test_oracle_physics.py`, `tests/test_cassie.py`,
`tests/test_elspider.py`), on all three topologies and through both launch shapes: `lg_compute_torques` + `lg_simulate` (the single-wave instance, one
sim.dt) and `lg_step_physics` (what every rollout runs: `decimation` substeps in one launch, helper waves).  Scenarios and arithmetic: `tests/physics_known_answers.py`.

  FREE FLIGHT (no contact switching, no chaos: the mass matrix, its per-leg Schur complement, the bias forces and the pose advance alone; 37 envs = partial
  workgroups on every instance with every lane-group position occupied; no env is left out of any bar):
    (a) COM acceleration g and conserved spin under internal torques: the error shrinks with dt as the oracle's does, and sits within 10 % of the oracle's
        own on the same inputs (both sides step the same discrete scheme, so their truncation errors coincide; 10 % is room for fp32 rounding over 160 substeps);
    (b) zero gravity, zero torques: momentum, energy and angular momentum at the oracle tests' bars, and within 10 % of the oracle's figure env by env;
    (c) one `lg_step_physics` launch = four x (`lg_compute_torques` + `lg_simulate`);
    (d) every entry of root / joint / body states against the oracle after one `simulate` and after one `step_physics`, at a bar taken from the oracle alone:
        16 x its own response to one-ulp input changes (floor 2e-6, the project's fp32 atol);
    (e) the slot an env sits in does not matter: 37 copies of one env give 37 bit-equal rows, in free flight and in a loaded stance.
  CONTACT: static stance (plane and a flat height grid), the friction limit, sliding deceleration, the momentum theorem over a landing -- the oracle tests'
  own scenarios and bars (physical statements, not fp32 ones).

Every printed figure goes to `hip_known_answers.json` in the directory LG_DUMP_DIR names (default: the system's temporary directory) when LG_DUMP_PARITY=1
(reviewed copy: `profiles/hip_known_answers.json`)."""
import json
import os

import numpy as np
import pytest

from tests import physics_known_answers as K

pytestmark = pytest.mark.gpu

N = K.N_FREE                # 16 / 8 / 16 envs per wave (quadruped / hexapod / biped): two full workgroups and a partial one, or four and a partial one
SEED = K.SEED_FREE          # the oracle alone meets the convergence bar of (a) with it on all three robots (tests/test_physics_known_answers.py)
MASS = {"anymal_c": 52.13485, "elspider_air": 30.50895708, "cassie": 30.468}      # the sums of the URDFs' <mass> tags
PATHS = ["simulate", "step_physics"]
FIGURES = {}
_CACHE = {}


def record(key, **figures):
    FIGURES[key] = figures
    print(key, json.dumps(figures))


@pytest.fixture(scope="module", autouse=True)
def _dump_figures():
    yield
    if os.environ.get("LG_DUMP_PARITY") != "1":       # (the reviewed copy lives in profiles/; a partial or failed run must not overwrite anything)
        return
    import tempfile
    root = os.environ.get("LG_DUMP_DIR") or tempfile.gettempdir()
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "hip_known_answers.json"), "w") as f:
        json.dump(dict(note="figures printed by tests/test_hip_physics_known_answers.py; `hip` is the device, `oracle` the CPU oracle on the same inputs",
                       figures=dict(sorted(FIGURES.items()))), f, indent=1)


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ (a)
def tumble(robot, side, dt, path):
    steps = int(round(0.2 / dt))
    sc = K.scenario(robot, N, control="T", dt=dt, free=True)
    root, dof, tq = K.tumbling_state(sc, SEED)
    rb0, out = K.free_run(sc, side, root, dof, sc.actions_for_torques(tq), steps, path)
    return K.free_flight_errors(sc, rb0, out["rigid_body_state"], steps * dt)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("robot", K.ROBOTS)
def test_free_fall_error_shrinks_with_dt_and_sits_at_the_oracles_level(robot, path):
    """(a) 0.2 s of tumbling under internal torques at sim.dt 0.005 and 0.00125: lin = |dP / M - g T|, ang = spin change / max(1, |spin|) per env in float64.
    An inconsistency between mass matrix, bias forces and pose advance does not shrink with dt; a wrong term that does is still above the oracle's level."""
    fig = {}
    for dt in (0.005, 0.00125):
        lin_o, ang_o, _ = cached(("tumble", robot, dt), lambda: tumble(robot, "oracle", dt, "simulate"))
        lin, ang, mass = tumble(robot, "hip", dt, path)
        fig[dt] = dict(hip_lin=float(lin.max()), hip_ang=float(ang.max()), oracle_lin=float(lin_o.max()), oracle_ang=float(ang_o.max()),
                       worst_env_lin=int(lin.argmax()), worst_env_ang=int(ang.argmax()))
        assert np.abs(mass - MASS[robot]).max() < 1e-3
    record(f"a/{robot}/{path}", **{f"dt={dt}": v for dt, v in fig.items()})
    c, f = fig[0.005], fig[0.00125]
    assert f["hip_lin"] <= 0.35 * c["hip_lin"] and f["hip_ang"] <= 0.35 * c["hip_ang"], fig
    for v in (c, f):
        assert v["hip_lin"] <= 1.10 * v["oracle_lin"], v
        assert v["hip_ang"] <= 1.10 * v["oracle_ang"], v


# ------------------------------------------------------------------------------------------------ (b)
def drift(robot, side, path):
    sc = K.scenario(robot, N, gravity=(0.0, 0.0, 0.0), control="T", free=True)
    root, dof, tq = K.drifting_state(sc, 1)
    rb0, out = K.free_run(sc, side, root, dof, sc.actions_for_torques(tq), 20, path)
    return K.conservation_errors(sc, rb0, out["rigid_body_state"])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("robot", K.ROBOTS)
def test_zero_gravity_conserves_momentum_energy_and_angular_momentum(robot, path):
    """(b) No gravity, no torques, 20 substeps: |dP| <= 2e-3 M, |dK| / K < 0.03, |dL| <= 0.02 max(1, |L|) per env (the oracle tests' bars), and each figure
    within 10 % of the oracle's for the same env."""
    ora = cached(("drift", robot), lambda: drift(robot, "oracle", "simulate"))
    hip = drift(robot, "hip", path)
    names = ("dP_over_M", "dK_over_K", "dL_rel")
    ratio = [h / o for h, o in zip(hip, ora)]
    record(f"b/{robot}/{path}", **{n: dict(hip=float(h.max()), oracle=float(o.max()), worst_ratio=float(r.max()), worst_env=int(r.argmax()))
                                   for n, h, o, r in zip(names, hip, ora, ratio)})
    for h, bar in zip(hip, (2e-3, 0.03, 0.02)):
        assert h.max() < bar, (robot, path, h.max(), int(h.argmax()))
    for n, r in zip(names, ratio):
        assert r.max() <= 1.10, (n, float(r.max()), int(r.argmax()))


# ------------------------------------------------------------------------------------------------ (d) and (c)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("robot", K.ROBOTS)
def test_every_entry_matches_the_oracle_in_free_flight(robot, path):
    """(d) Tumbling at speed, no contact: every entry of root_states, dof_state and rigid_body_state of all 37 envs after one `simulate` / one `step_physics`
    within max(16 y, 2e-6) of the oracle, y = the oracle's own largest response to one-ulp changes of its inputs (`yardstick`)."""
    base, y = cached(("yardstick", robot, path), lambda: K.yardstick(robot, path))
    sc, root, dof, act = K.parity_inputs(robot)
    hip = K.one_call(sc, "hip", root, dof, act, path)
    bars = K.bars_of(y)
    fig, miss = {}, []
    for name in K.STATE:
        err = K.relative_error(hip[name], base[name]).reshape(N, -1)
        fig[name] = dict(y=y[name], bar=bars[name], err=float(err.max()), ratio_to_y=float(err.max() / max(y[name], 1e-30)), worst_env=int(err.max(axis=1).argmax()))
        if not err.max() <= bars[name]:
            miss.append(name)
    record(f"d/{robot}/{path}", **fig)
    assert not miss, {name: fig[name] for name in miss}


@pytest.mark.parametrize("robot", K.ROBOTS)
def test_one_launch_equals_four_substeps(robot):
    """(c) `lg_step_physics` against four x (`lg_compute_torques` + `lg_simulate`) from the same tumbling state: root_states, dof_state, rigid_body_state, torques.

    The six-joint (chain) instance is meant to be bit-equal and is held to it: its helper waves only detect contacts, every piece of the dynamics runs on the
    main wave through the one text of `chain_substep` (`csrc/lg_chain_body.h`) whatever the mode.
    The three-joint instances with helper waves (what `lg_step_physics` launches) are not, and nothing in the code promises it: that launch is another instance
    of `physics_kernel` than `lg_simulate`'s (helper waves, no in-line bias / detection, another feature set), the build leaves the contraction of sums into
    fused multiply-adds to the compiler per instance, and the two come out an ulp apart per substep.  Narrowed down on the device: (1) the single-wave policy-step
    instance (`LG_SPLIT=0`) IS `lg_simulate` bit for bit over the four substeps -- the test below --, so the substep loop, the state carried in registers and the
    torques recomputed per substep are not it; (2) one substep at rest in zero gravity, where the leg bias that helper wave 1 supplies is exactly zero, still
    differs by 1.2e-7 in the joint states, so it is not a helper wave's product either: it is the main wave's own `physics_substep` arithmetic (mass matrix,
    Schur complement, velocity update) as compiled into the helper-wave instance.  Which instruction is contracted differently was not traced.
    So there the states are held to the bar of (d) -- 16 x the oracle's response to one-ulp input changes over the same four substeps --, the torques
    (`control_type = "T"`: action x scale, clipped) to equality; measured: 1.3e-7 / 5.4e-7 / 7.2e-7 (quadruped: root, joint, body states) and 1.7e-7 / 9.9e-7 /
    1.0e-5 (hexapod) against bars of 3e-5 .. 6e-4."""
    _, y = cached(("yardstick", robot, "step_physics"), lambda: K.yardstick(robot, "step_physics"))
    sc, root, dof, act = K.parity_inputs(robot)
    one = K.one_call(sc, "hip", root, dof, act, "step_physics")
    four = K.free_run(sc, "hip", root, dof, act, sc.decimation, "simulate")[1]
    bars = K.bars_of(y)
    fig = {name: dict(bar=bars[name], err=float(K.relative_error(one[name], four[name]).max()), bit_equal=bool(np.array_equal(one[name], four[name]))) for name in K.STATE}
    record(f"c/{robot}", **fig)
    assert np.array_equal(one["torques"], four["torques"])
    for name in K.STATE:
        assert fig[name]["err"] <= bars[name], (name, fig[name])
        assert robot != "cassie" or fig[name]["bit_equal"], (name, fig[name])


@pytest.mark.parametrize("robot", K.ROBOTS)
def test_single_wave_launch_equals_four_substeps_bit_for_bit(robot, monkeypatch):
    """(c) without helper waves (`LG_SPLIT=0`: the single-wave policy-step instance, the checker of the helper-wave path): the launch's substep loop -- state kept
    in registers, torques recomputed in front of every substep -- against four x (`lg_compute_torques` + `lg_simulate`), every tensor bit for bit on all three
    topologies.  The two instances differ in MODE alone."""
    monkeypatch.setenv("LG_SPLIT", "0")
    sc, root, dof, act = K.parity_inputs(robot)
    one = K.one_call(sc, "hip", root, dof, act, "step_physics")
    four = K.free_run(sc, "hip", root, dof, act, sc.decimation, "simulate")[1]
    for name in K.STATE + ["torques"]:
        assert np.array_equal(one[name], four[name]), (name, float(K.relative_error(one[name], four[name]).max()))


# ------------------------------------------------------------------------------------------------ (e)
def assert_rows_equal_env0(sim, names, what):
    for name in names:
        a = sim.get(name).reshape(N, -1)
        same = (a.view(np.uint32) == a[:1].view(np.uint32)).all(axis=1)
        assert same.all(), f"{what}: {name} of envs {np.flatnonzero(~same).tolist()} differs from env 0's"


@pytest.mark.parametrize("robot", K.ROBOTS)
def test_the_slot_an_env_sits_in_does_not_matter_in_free_flight(robot):
    """(e) Env 0's tumbling state and torques in all 37 slots: after `step_physics`, and after `simulate`, every env's rows are env 0's bit for bit -- a cross-leg
    reduction that is wrong in one lane group, or a partial workgroup that computes on something else, shows here."""
    sc, root, dof, act = K.parity_inputs(robot)
    root[:], dof[:], act[:] = root[0], dof[0], act[0]
    for path in PATHS:
        sim = sc.sim("hip")
        K.place(sim, root, dof)
        K.advance(sim, sc, act, 1 if path == "simulate" else sc.decimation, path)
        assert_rows_equal_env0(sim, K.STATE + ["torques", "contact_forces"], f"{robot} / {path}")
        assert np.abs(sim.get("root_states")[0] - root[0]).max() > 1e-4            # (it did move)
        sim.close()


@pytest.mark.parametrize("robot", K.ROBOTS)
def test_the_slot_an_env_sits_in_does_not_matter_in_a_loaded_stance(robot):
    """(e) on the plane: env 0 after settling on its feet (the static stance below; the biped, which has no static stance without a policy, ten policy steps
    after its reset, both toes loaded), copied into every slot, positions included; one `step_physics`: contact forces too are env 0's bit for bit."""
    sc = K.scenario(robot, N, control="P")
    sim = sc.sim("hip")
    sim.reset_idx()
    root = sim.get("root_states"); root[:, 7:13] = 0
    sim.set("root_states", root); sim.refresh()
    z = np.zeros((N, sc.nd), np.float32)
    for _ in range(10 if robot == "cassie" else 100):
        sim.step(z)
    root, dof = sim.get("root_states"), sim.get("dof_state")
    assert sim.get("contact_forces")[0, :, 2].sum() > 0.5 * sc.mass * K.G and not sim.get("reset_buf")[0]
    sim.close()
    root[:], dof[:] = root[0], dof[0]
    sim = sc.sim("hip")
    K.place(sim, root, dof)
    sim.step_physics(z)
    assert_rows_equal_env0(sim, K.STATE + ["torques", "contact_forces"], robot)
    feet = list(sc.model["feet_indices"])
    assert (sim.get("contact_forces")[0, feet, 2] > 1.0).all()
    sim.close()


# ------------------------------------------------------------------------------------------------ contact known answers
@pytest.mark.parametrize("terrain", ["plane", "grid"])
@pytest.mark.parametrize("solver", K.SOLVERS, ids=lambda s: "-".join(s))
@pytest.mark.parametrize("robot", ["anymal_c", "elspider_air"])
def test_static_stance_supports_the_weight(robot, solver, terrain):
    """100 policy steps of zero actions: the summed vertical contact force is (m + payload) g within 3 %, the base rests in the oracle test's height band (the
    quadruped: and twist band), no foot sinks below -5 mm, every foot carries more than the stance threshold of 1 N, nobody resets -- on the plane and, through
    the grid's contact path, on a height grid whose cells are all equal.  (The biped is absent: with zero actions it topples within a second on the oracle too.)"""
    sc = K.scenario(robot, len(K.STANCE[robot]["payload"]), control="P", solver=solver, grid=terrain == "grid")
    sim = sc.sim("hip")
    K.stance_start(sim, sc)
    fig = K.stance_figures(sim, sc, K.stance_run(sim, sc))
    sim.close()
    record(f"stance/{robot}/{'-'.join(solver)}/{terrain}", **fig)
    K.check_stance(fig, sc)


FRICTION_CASES = [("anymal_c", s) for s in K.SOLVERS] + [("elspider_air", ("tgs", "pyramid")), ("elspider_air", ("pgs", "cone")), ("cassie", ("tgs", "pyramid"))]


@pytest.mark.parametrize("robot,solver", FRICTION_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(v))
def test_friction_limit_holds_on_every_contact_body(robot, solver):
    """60 policy steps of random actions, 8 robots of friction 0.2 .. 1.2: on every body and step |f_t| <= mu f_n (cone) or each tangential axis on its own
    (PhysX's box, pyramid), and no contact pulls.  (The hexapod and the biped with the solver settings their oracle tests use; self-collision off: its forces
    are internal, not the terrain's.)"""
    sc = K.scenario(robot, 8, control="P", solver=solver, self_collisions=False)
    sim = sc.sim("hip")
    worst, fn_min = K.friction_limit_run(sim, sc, solver)
    sim.close()
    record(f"friction_limit/{robot}/{'-'.join(solver)}", worst_excess=worst, lowest_normal_force=fn_min)
    assert fn_min >= -1e-3
    assert worst < 1e-2


@pytest.mark.parametrize("solver", K.SOLVERS, ids=lambda s: "-".join(s))
def test_sliding_friction_decelerates_at_mu_g(solver):
    sc = K.scenario("anymal_c", 1, control="P", solver=solver)
    sim = sc.sim("hip")
    dec = K.sliding_run(sim, sc)
    sim.close()
    record(f"sliding/anymal_c/{'-'.join(solver)}", deceleration_over_g=dec / K.G)
    assert 0.35 * K.G < dec < 0.75 * K.G


@pytest.mark.parametrize("robot", K.ROBOTS)
def test_contact_forces_account_for_the_momentum_of_a_landing(robot):
    """Momentum theorem over a landing, substep by substep through `lg_simulate`: dP = sum (contact forces - m g) dt within 2 % of the weight's impulse, peak
    load above 2 m g.  Ties the device's contact solve, mass matrix and force report together without the oracle."""
    sc = K.scenario(robot, 4, control="T", free=True)
    sim = sc.sim("hip")
    dP, impulse, peak = K.landing_run(sim, sc)
    sim.close()
    tol = 0.02 * sc.mass * K.G * 100 * sc.sim_dt
    record(f"landing/{robot}", peak_over_weight=(peak / (sc.mass * K.G)).tolist(), worst_mismatch_over_tolerance=float(np.abs(dP - impulse).max() / tol))
    K.check_landing(sc, dP, impulse, peak)
