"""`lg_runner_collect_distillation` / `lg_runner_collect_distillation_recurrent` (include/lgrunner_distill.h) through `rl.collect_distillation_tracked`
on twin `anymal_c_rough_student` envs of one seed (3 x 4 heightfield tiles, 64 envs, episodes of 4 policy steps so that time-outs and resets fall
inside the rollout, staggered episode clocks): the one call against the host loop -- `policy.act_and_teach(obs, priv)`, `env.step`, the two
normalisers, `policy.reset(dones)` (`on_policy_runner.py:395-431`, `distillation.py:89-105`) -- bit for bit in every row, in both normalisers'
states, counts and carried rows, in the env's rows and history, in the episode tracker and in the student memory."""
import pytest
import torch

from tests.test_hip_distillation import _python_step
from tests.test_hip_runner_collect import episode_restatement, same
from tests.test_hip_runner_collect_privileged import normalisers, same_normaliser, twins

pytestmark = pytest.mark.gpu
N, OS, OT = 64, 144, 235
DROWS = ("observations", "privileged_observations", "actions", "privileged_actions", "rewards", "dones")
TROWS = DROWS + ("raw_rewards", "episode_extras")
CFG = dict(student_hidden_dims=[64, 32], teacher_hidden_dims=[48], activation="elu", init_noise_std=0.7, rnn_type="lstm", rnn_hidden_dim=64, rnn_num_layers=1)


def policy(recurrent, num_obs=OS, num_teacher_obs=OT, seed=11):
    from extended_legged_gym_amd.rl import NativeStudentTeacher, NativeStudentTeacherRecurrent
    from extended_legged_gym_amd.rl.distillation_runner import initial_distillation_state_dict
    sd = initial_distillation_state_dict("StudentTeacherRecurrent" if recurrent else "StudentTeacher", num_obs, num_teacher_obs, 12, CFG, 3)
    if recurrent:
        return NativeStudentTeacherRecurrent(sd, activation="elu", rnn_type="lstm", device="cuda:0", seed=seed)
    return NativeStudentTeacher(sd, activation="elu", device="cuda:0", seed=seed)


def host_loop(env, pol, T, norm_s=None, norm_t=None, obs=None, priv=None, u=None):
    """The runner's distillation loop on the host.  Returns the rollout dict and the two rows after the last step."""
    rows = {k: [] for k in TROWS}
    obs = env.get_observations() if obs is None else obs
    priv = env.get_privileged_observations() if priv is None else priv
    before = None
    if pol.is_recurrent:
        pol.memory_s.ensure_state(N)
        before = tuple(h.clone() for h in pol.memory_s.hidden_states)
    for t in range(T):
        a, teach = pol.act_and_teach(obs, priv)          # Distillation.act (distillation.py:89-96)
        rows["observations"].append(obs.clone()); rows["privileged_observations"].append(priv.clone())
        rows["actions"].append(a.clone()); rows["privileged_actions"].append(teach.clone())
        obs, priv, rew, dones, infos = _python_step(env, a, u[t]) if u is not None else env.step(a)
        obs = norm_s(obs) if norm_s is not None else obs.clone()          # on_policy_runner.py:425-427
        priv = norm_t(priv) if norm_t is not None else priv.clone()
        rows["rewards"].append(rew.clone().view(-1, 1)); rows["raw_rewards"].append(rew.clone().view(-1, 1))          # distillation.py:98-101: no bootstrap
        rows["dones"].append(dones.float().view(-1, 1)); rows["episode_extras"].append(env.core.t["extras_episode"].clone())
        pol.reset(dones)          # distillation.py:105
    out = {k: torch.stack(v) for k, v in rows.items()}
    out["hidden_states"] = before
    return out, obs, priv


@pytest.mark.parametrize("recurrent,T,noise", [(False, 5, False), (True, 3, False), (False, 5, True)], ids=["feedforward", "lstm64", "feedforward-noise"])
def test_one_call_matches_the_host_loop(recurrent, T, noise):
    from extended_legged_gym_amd.rl import EpisodeTracker, collect_distillation_tracked
    envs = twins(noise)
    pols = [policy(recurrent) for _ in range(2)]
    norms = [normalisers() for _ in range(2)]
    tracker = EpisodeTracker(N, "cuda:0")
    tracker.cur_reward_sum[:] = torch.linspace(-1.0, 1.0, N, device="cuda")
    tracker.cur_episode_length[:] = (torch.arange(N, device="cuda") % 3).float()
    sum0, len0 = tracker.cur_reward_sum.clone(), tracker.cur_episode_length.clone()
    u = torch.rand(2 * T, N, OS, generator=torch.Generator().manual_seed(9)).cuda() if noise else None
    raw_s, raw_t = envs[1].get_observations().clone(), envs[1].get_privileged_observations().clone()
    # ---- first collection: row 0 of both streams raw and not counted
    ref, car_s, car_t = host_loop(envs[0], pols[0], T, *norms[0], u=u)
    out = collect_distillation_tracked(envs[1], pols[1], T, obs_normalizer=norms[1][0], privileged_obs_normalizer=norms[1][1], episode_tracker=tracker,
                                       noise_uniforms=u[:T] if noise else None)
    torch.cuda.synchronize()
    assert out["observations"].shape == (T, N, OS) and out["privileged_observations"].shape == (T, N, OT)
    same(ref, out, TROWS)
    assert torch.equal(out["raw_rewards"], out["rewards"])
    assert torch.equal(out["observations"][0], raw_s) and torch.equal(out["privileged_observations"][0], raw_t)
    for k in range(2):
        same_normaliser(norms[0][k], norms[1][k], T * N)
    assert torch.equal(norms[1][0].carried_row(N), car_s) and torch.equal(norms[1][1].carried_row(N), car_t)
    assert torch.equal(envs[0].obs_buf, envs[1].obs_buf) and torch.equal(envs[0].obs_history, envs[1].obs_history)
    assert torch.equal(envs[0].get_privileged_observations(), envs[1].get_privileged_observations())          # the env's own row stays raw
    assert not torch.equal(envs[1].obs_buf, car_s) and pols[0]._call == pols[1]._call == T
    assert envs[0].common_step_counter == envs[1].common_step_counter
    if noise:
        assert not torch.equal(envs[1].obs_buf[:, :48], envs[1].get_privileged_observations()[:, :48])
    else:
        assert torch.equal(envs[1].obs_buf[:, :48], envs[1].get_privileged_observations()[:, :48])
    if recurrent:
        got = out["hidden_states"]
        assert got[1] is None and all(torch.equal(x, y) for x, y in zip(ref["hidden_states"], got[0]))
        for x, y in zip(pols[0].memory_s.hidden_states, pols[1].memory_s.hidden_states):
            assert torch.equal(x, y) and float(x.abs().sum()) > 0
    # time-outs and resets fell inside the rollout
    assert 0 < float(out["dones"].sum()) < T * N
    rb, lb, sum1, len1 = episode_restatement(ref["raw_rewards"][..., 0], ref["dones"][..., 0], sum0, len0)
    assert torch.equal(tracker.cur_reward_sum, sum1) and torch.equal(tracker.cur_episode_length, len1)
    tracker.extend(out["dones"], out["ep_return"], out["ep_length"])
    assert len(rb) > 0 and list(tracker.rewbuffer) == rb[-100:] and list(tracker.lenbuffer) == lb[-100:]
    # ---- second collection on the same objects: row 0 of both streams is the carried row
    ref2, car_s2, car_t2 = host_loop(envs[0], pols[0], T, *norms[0], obs=car_s, priv=car_t, u=u[T:] if noise else None)
    out2 = collect_distillation_tracked(envs[1], pols[1], T, obs_normalizer=norms[1][0], privileged_obs_normalizer=norms[1][1], episode_tracker=tracker,
                                        noise_uniforms=u[T:] if noise else None)
    assert torch.equal(out2["observations"][0], car_s) and torch.equal(out2["privileged_observations"][0], car_t)
    same(ref2, out2, TROWS)
    for k in range(2):
        same_normaliser(norms[0][k], norms[1][k], 2 * T * N)
    assert torch.equal(norms[1][0].carried_row(N), car_s2) and torch.equal(norms[1][1].carried_row(N), car_t2)
    assert torch.equal(envs[0].obs_history, envs[1].obs_history) and torch.equal(envs[0].obs_buf, envs[1].obs_buf)
    if recurrent:
        for x, y in zip(pols[0].memory_s.hidden_states, pols[1].memory_s.hidden_states):
            assert torch.equal(x, y)


@pytest.mark.parametrize("student,teacher", [(True, False), (False, True)], ids=["student-only", "teacher-only"])
def test_one_normaliser_leaves_the_other_stream_raw(student, teacher):
    from extended_legged_gym_amd.rl import collect_distillation_tracked
    envs, T = twins(), 5
    pols = [policy(False) for _ in range(2)]
    norms = [normalisers(student, teacher) for _ in range(2)]
    ref, last_s, last_t = host_loop(envs[0], pols[0], T, *norms[0])
    out = collect_distillation_tracked(envs[1], pols[1], T, obs_normalizer=norms[1][0], privileged_obs_normalizer=norms[1][1])
    same(ref, out, DROWS)
    assert "raw_rewards" not in out
    for k, last in enumerate((last_s, last_t)):
        if norms[1][k] is not None:
            same_normaliser(norms[0][k], norms[1][k], T * N)
            assert torch.equal(norms[1][k].carried_row(N), last)
    assert torch.equal(envs[0].obs_buf, envs[1].obs_buf) and torch.equal(envs[0].obs_history, envs[1].obs_history)
    raw_s, raw_t = envs[1].obs_buf.clone(), envs[1].get_privileged_observations().clone()
    ref2, _, _ = host_loop(envs[0], pols[0], 2, *norms[0], obs=last_s, priv=last_t)
    out2 = collect_distillation_tracked(envs[1], pols[1], 2, obs_normalizer=norms[1][0], privileged_obs_normalizer=norms[1][1])
    same(ref2, out2, DROWS)
    # the stream without a handle stays raw: its row 0 is the env's own row again, the other stream's is the carried (normalised) one
    assert torch.equal(out2["observations"][0], raw_s) != student and torch.equal(out2["privileged_observations"][0], raw_t) != teacher


def test_eval_mode_normalises_and_leaves_the_statistics():
    from extended_legged_gym_amd.rl import collect_distillation_tracked
    envs, T = twins(), 3
    pols = [policy(False) for _ in range(2)]
    norms = [normalisers() for _ in range(2)]
    g = torch.Generator().manual_seed(4)
    for width, k in ((OS, 0), (OT, 1)):          # statistics that are not the initial 0 / 1
        batch = (torch.randn(256, width, generator=g) * 0.5 + 0.1).cuda()
        for pair in norms:
            pair[k].update(batch)
            pair[k].eval()
    states = [n.get_state() for n in norms[1]]
    ref, last_s, last_t = host_loop(envs[0], pols[0], T, *norms[0])
    out = collect_distillation_tracked(envs[1], pols[1], T, obs_normalizer=norms[1][0], privileged_obs_normalizer=norms[1][1])
    same(ref, out, DROWS)
    assert torch.equal(norms[1][0].carried_row(N), last_s) and torch.equal(norms[1][1].carried_row(N), last_t)
    assert torch.equal(norms[1][0].carried_row(N), norms[1][0](envs[1].obs_buf))          # the rows ARE normalised: the carried row is norm(raw last row)
    for n, before in zip(norms[1], states):
        after = n.get_state()
        assert after[3] == before[3] == 256 and all((p == q).all() for p, q in zip(after[:3], before[:3]))
    norms[1][0].train()          # one handle training, the other not: refused on the host
    with pytest.raises(ValueError, match="different modes"):
        collect_distillation_tracked(envs[1], pols[1], T, obs_normalizer=norms[1][0], privileged_obs_normalizer=norms[1][1])


@pytest.mark.parametrize("recurrent", [False, True], ids=["feedforward", "lstm64"])
def test_no_hooks_is_collect_distillation_bit_for_bit(recurrent):
    from extended_legged_gym_amd.rl import collect_distillation, collect_distillation_tracked
    envs, T = twins(), 5
    pols = [policy(recurrent) for _ in range(2)]
    a = collect_distillation(envs[0], pols[0], T)
    b = collect_distillation_tracked(envs[1], pols[1], T)
    assert sorted(a) == sorted(b)
    same(a, b, DROWS)
    assert float(a["dones"].sum()) > 0 and pols[1]._call == T and envs[0].common_step_counter == envs[1].common_step_counter
    assert torch.equal(envs[0].obs_buf, envs[1].obs_buf) and torch.equal(envs[0].obs_history, envs[1].obs_history)
    if recurrent:
        assert all(torch.equal(x, y) for x, y in zip(a["hidden_states"][0], b["hidden_states"][0]))
        assert all(torch.equal(x, y) for x, y in zip(pols[0].memory_s.hidden_states, pols[1].memory_s.hidden_states))


def test_refusals_carry_their_reason():
    from extended_legged_gym_amd.rl import NativeEmpiricalNormalization, collect_distillation_tracked
    student, flat = twins()[0], twins(task="anymal_c_flat")[0]
    before = student.obs_history.clone()
    good = policy(False)
    # everything lg_collect_distillation refuses
    with pytest.raises(RuntimeError, match="lg_runner_collect_distillation: the student's input width is not H x W of the history layer"):
        collect_distillation_tracked(student, policy(False, 96, OT), 2)
    with pytest.raises(RuntimeError, match="lg_runner_collect_distillation: network widths do not match the env"):
        collect_distillation_tracked(student, policy(False, OS, OS), 2)
    with pytest.raises(RuntimeError, match="lg_runner_collect_distillation: without a history layer the student reads a prefix"):
        collect_distillation_tracked(flat, policy(False, 60, 48), 2)
    # a normaliser whose width is not its stream's
    wide, narrow = NativeEmpiricalNormalization([OT], device="cuda:0"), NativeEmpiricalNormalization([OS], device="cuda:0")
    with pytest.raises(RuntimeError, match="lg_runner_collect_distillation: the student's normaliser does not have the student's input width"):
        collect_distillation_tracked(student, good, 2, obs_normalizer=wide)
    with pytest.raises(RuntimeError, match="lg_runner_collect_distillation: the teacher's normaliser does not have the env's observation width"):
        collect_distillation_tracked(student, good, 2, privileged_obs_normalizer=narrow)
    with pytest.raises(RuntimeError, match="lg_runner_collect_distillation_recurrent: the student's normaliser does not have"):
        collect_distillation_tracked(student, policy(True), 2, obs_normalizer=wide)          # (the recurrent entry point: the same loop)
    # one handle for both streams (a 48-wide env whose student reads the whole row)
    both = NativeEmpiricalNormalization([48], device="cuda:0")
    with pytest.raises(RuntimeError, match="lg_runner_collect_distillation: the student and the teacher need a normaliser each"):
        collect_distillation_tracked(flat, policy(False, 48, 48), 2, obs_normalizer=both, privileged_obs_normalizer=both)
    # handles on another device than the networks (where there is one)
    if torch.cuda.device_count() > 1:
        far = NativeEmpiricalNormalization([OS], device="cuda:1")
        with pytest.raises(RuntimeError, match="lg_runner_collect_distillation: a normaliser is on another device than the networks"):
            collect_distillation_tracked(student, good, 2, obs_normalizer=far)
    # nothing was launched: no row counted, no carried row, no history moved, no sampling call drawn
    for n in (wide, narrow, both):
        assert n.get_state()[3] == 0 and n.carried_row(N) is None
    assert torch.equal(student.obs_history, before) and good._call == 0
