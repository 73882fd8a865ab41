"""`learn()` of the two native runners (`on_policy_runner.py:347-486`) on the CPU: the order of collect / update / save / reward stage, what the
writer gets, and what is left behind.  The runner is made with `object.__new__` and plain attributes, over a stub env, a stub algorithm and a
`_collect` that returns CPU rows for T = 2 with one finished episode, so no library is loaded."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from extended_legged_gym_amd.rl import NativeDistillationRunner, NativeOnPolicyRunner
from extended_legged_gym_amd.rl.distillation_runner import NO_TEACHER_MESSAGE

RUNNERS = [NativeOnPolicyRunner, NativeDistillationRunner]
T, N = 2, 3
EPISODE_RETURN, EPISODE_LENGTH = 5.0, 7.0
PER_ITERATION_TAGS = {"Episode/view", "Episode/own", "Loss/a", "Loss/learning_rate", "Policy/mean_noise_std", "Perf/total_fps", "Perf/collection time",
                      "Perf/learning_time", "Train/mean_reward", "Train/mean_episode_length"}
TIME_TAGS = ["Train/mean_reward/time", "Train/mean_episode_length/time"]          # their step is the run's wall-clock time


def make_runner(cls, log_dir, loaded_teacher=True, disable_logs=False):
    events = []
    ex = torch.tensor([0.25, 0.5])
    env = SimpleNamespace(num_envs=N, episode_length_buf=torch.full((N,), -1, dtype=torch.long), max_episode_length=40.0,
                          extras={"episode": {"view": ex[1], "own": torch.tensor(4.0)}}, core=SimpleNamespace(t={"extras_episode": ex}), reward_scales_stage=1)
    env.update_reward_scales = lambda mean: events.append(("stage", mean)) or True
    policy = SimpleNamespace(std=torch.full((4,), 0.5), loaded_teacher=loaded_teacher)
    alg = SimpleNamespace(policy=policy, learning_rate=1.0e-3, update=lambda rollout: events.append("update") or {"a": 0.125})
    runner = object.__new__(cls)
    runner.__dict__.update(env=env, alg=alg, device="cpu", log_dir=log_dir, disable_logs=disable_logs, writer=None, cfg={"multi_stage_rewards": True},
                           num_steps_per_env=T, save_interval=1, tot_timesteps=0, tot_time=0.0, current_learning_iteration=0, layered=False, privileged=False,
                           empirical_normalization=False, obs_normalizer=None, privileged_obs_normalizer=None, resumed=False,
                           _host_obs=torch.ones(N, 2), _host_priv=torch.ones(N, 2), _host_episode=None)
    trackers = []

    def collect(tracker):
        events.append("collect")
        trackers.append((tracker, len(tracker.rewbuffer), tracker.cur_reward_sum.clone()))
        tracker.cur_reward_sum.fill_(3.0)
        dones = torch.zeros(T, N, 1)
        dones[1, 2] = 1.0
        return dict(dones=dones, ep_return=EPISODE_RETURN * dones, ep_length=EPISODE_LENGTH * dones, episode_extras=torch.tensor([[0.0, 1.0], [0.0, 3.0]]))
    runner._collect = collect
    runner.save = lambda path, infos=None: events.append(("save", os.path.basename(path)))
    return runner, events, trackers


def scalars(log_dir):
    return [json.loads(line) for line in open(os.path.join(log_dir, "scalars.jsonl"))]


@pytest.mark.parametrize("cls", RUNNERS)
def test_learn_collects_updates_saves_and_stages_in_the_reference_order(cls, tmp_path):
    runner, events, trackers = make_runner(cls, str(tmp_path))
    runner.learn(2, init_at_random_ep_len=True)
    iteration = lambda it: ["collect", "update", ("save", f"model_{it}.pt"), ("stage", EPISODE_RETURN)]          # noqa: E731
    assert events == iteration(0) + iteration(1) + [("save", "model_1.pt")]
    assert runner.current_learning_iteration == 1 and runner.tot_timesteps == 2 * T * N          # the reference's `= it`
    assert runner._host_obs is None and runner._host_priv is None
    buf = runner.env.episode_length_buf
    assert bool((buf >= 0).all()) and bool((buf < 40).all())
    # one tracker for the whole run; the stage change empties the buffer and the live sums before the next collection
    assert trackers[0][0] is trackers[1][0] and [t[1] for t in trackers] == [0, 0]
    assert torch.equal(trackers[1][2], torch.zeros(N)) and list(trackers[0][0].rewbuffer) == [] and list(trackers[0][0].lenbuffer) == [EPISODE_LENGTH] * 2
    log = scalars(str(tmp_path))
    for it in (0, 1):
        rows = {r["tag"]: r["value"] for r in log if r["step"] == it and r["tag"] not in TIME_TAGS}
        assert set(rows) == PER_ITERATION_TAGS
        assert rows["Episode/view"] == 2.0 and rows["Episode/own"] == 4.0 and rows["Loss/a"] == 0.125 and rows["Loss/learning_rate"] == 1.0e-3
        assert rows["Policy/mean_noise_std"] == 0.5 and rows["Train/mean_reward"] == EPISODE_RETURN and rows["Train/mean_episode_length"] == EPISODE_LENGTH
    timed = [r for r in log if r["tag"] in TIME_TAGS]
    assert len(log) == 2 * len(PER_ITERATION_TAGS) + len(timed) and [r["tag"] for r in timed] == TIME_TAGS * 2
    assert all(isinstance(r["step"], float) and 0.0 <= r["step"] <= runner.tot_time for r in timed)
    assert [r["value"] for r in timed] == [EPISODE_RETURN, EPISODE_LENGTH] * 2
    assert os.listdir(str(tmp_path)) == ["scalars.jsonl"]


@pytest.mark.parametrize("cls", RUNNERS)
@pytest.mark.parametrize("silent", ["no_log_dir", "disable_logs"])
def test_without_a_log_dir_or_with_logs_disabled_nothing_is_saved_or_written(cls, silent, tmp_path):
    runner, events, _ = make_runner(cls, None if silent == "no_log_dir" else str(tmp_path), disable_logs=silent == "disable_logs")
    runner.learn(2)
    assert events == ["collect", "update", ("stage", EPISODE_RETURN)] * 2
    assert runner.writer is None and os.listdir(str(tmp_path)) == [] and runner.current_learning_iteration == 1 and runner.tot_timesteps == 0
    assert bool((runner.env.episode_length_buf == -1).all())


def test_distillation_without_a_teacher_raises_before_anything_is_opened(tmp_path):
    runner, events, _ = make_runner(NativeDistillationRunner, str(tmp_path), loaded_teacher=False)
    with pytest.raises(ValueError) as e:
        runner.learn(2)
    assert str(e.value) == NO_TEACHER_MESSAGE
    assert events == [] and runner.writer is None and os.listdir(str(tmp_path)) == []
