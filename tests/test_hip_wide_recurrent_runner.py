"""GPU: `NativeOnPolicyRunner` with `policy_class_name = "ActorCriticRecurrent"` on `elspider_air_rough_raycast`, rows of 66 proprioceptive columns +
512 ray distances = 578: both memories are wide ones (`lg_rnn_create_wide`), collected by the host loop (`runner.sensor_collection = "host"`) and by
the sensor collector (`"native"`), trained by `NativeRecurrentPPO`.  Env sizes of tests/test_hip_wide_runner.py: the small terrain, 32 envs, 4 steps
per env.  Everything is compared with `torch.equal`: the two collection modes launch the same kernels on the same rows."""
import copy
import math

import pytest
import torch

from tests.test_env_api import make
from tests.test_hip_estimator import ENV_OVER
from tests.test_hip_sensor_collection import _end_soon, _same
from tests.test_hip_wide_runner import N, T, TASK, train_cfg

pytestmark = pytest.mark.gpu


def recurrent_cfg(mode, normalization):
    cfg = train_cfg(empirical_normalization=normalization, policy_class_name="ActorCriticRecurrent", sensor_collection=mode)
    cfg["policy"].pop("class_name", None)
    cfg["policy"].update(rnn_hidden_size=64, rnn_type="lstm", rnn_num_layers=1)
    return cfg


def _carry_over(fresh, lived):
    """What a checkpoint does not hold and an uninterrupted run keeps: the policy's draw counter and the memories' state."""
    new, old = fresh.alg.policy, lived.alg.policy
    new._call = old._call
    for mem, src in ((new.memory_a, old.memory_a), (new.memory_c, old.memory_c)):
        mem.set_state(src.hidden_states)


@pytest.mark.parametrize("normalization", [False, True], ids=["plain", "empirical_normalization"])
def test_recurrent_runner_on_the_raycast_task_host_and_native(tmp_path, normalization):
    from extended_legged_gym_amd import abi
    from extended_legged_gym_amd.rl import EpisodeTracker, NativeOnPolicyRunner
    from extended_legged_gym_amd.rl.runner import initial_state_dict
    modes = ("host", "native")
    cfgs = [recurrent_cfg(m, normalization) for m in modes]
    envs = [make(TASK, N, **ENV_OVER) for _ in modes]
    runners = [NativeOnPolicyRunner(e, c, log_dir=str(tmp_path / m), device="cuda:0") for e, c, m in zip(envs, cfgs, modes)]
    for r, m in zip(runners, modes):
        pol = r.alg.policy
        assert r.sensor_collection == m and r.layered == (m == "host") and pol.is_recurrent
        assert pol.memory_a.input_size == pol.memory_c.input_size == 578 > abi.RNN_MAX_WIDTH and pol.actor.dims[0] == 64
    for e in envs:
        _end_soon(e)
    # ---- the collected rows of the two modes (twice: the carried rows and the memories cross a call boundary)
    trackers = [EpisodeTracker(N, "cuda:0") for _ in modes]
    ones = 0
    for rnd in range(2):
        a, b = (r._collect(t) for r, t in zip(runners, trackers))
        assert sorted(a) == sorted(b) and a["observations"].shape == (T, N, 578)
        for k in a:
            _same(a[k], b[k], f"{k}, collection {rnd}")
        assert float(a["observations"][..., 66:].abs().max()) > 0.0 and float(a["hidden_states_a"][0][-1].abs().max()) > 0.0
        ones += int(a["dones"].sum())
    assert ones >= 8          # the envs that were about to time out did, inside the window
    # ---- two iterations each: finite losses, and the same parameters
    losses = [[], []]
    for r, log in zip(runners, losses):
        update = r.alg.update
        r.alg.update = lambda rollout, update=update, log=log: log.append(update(rollout)) or log[-1]
        r.learn(2)
    print("losses, host:", losses[0], "native:", losses[1])
    assert all(len(log) == 2 and all(math.isfinite(float(v)) for d in log for v in d.values()) for log in losses) and losses[0] == losses[1]
    sds = [r.alg.state_dict() for r in runners]
    sd0 = initial_state_dict("ActorCriticRecurrent", 578, envs[0].num_actions, cfgs[0]["policy"], cfgs[0]["seed"])
    assert all(torch.equal(sds[0][k], sds[1][k]) for k in sds[0])
    moved = (sds[1]["memory_a.rnn.weight_ih_l0"] - sd0["memory_a.rnn.weight_ih_l0"]).abs()
    assert float(moved[:, 66:512].max()) > 0.0 and float(moved[:, 512:].max()) > 0.0          # ray columns on both sides of the slab edge train
    # ---- the checkpoint: rsl_rl's layout; save -> load into a new runner -> one more iteration = the uninterrupted run's bits
    path = str(tmp_path / "native" / "model_1.pt")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert [k for k in ck if "norm" not in k] == ["model_state_dict", "optimizer_state_dict", "iter", "infos"] and ck["iter"] == 1
    assert ("obs_norm_state_dict" in ck) == normalization and ck["model_state_dict"]["memory_a.rnn.weight_ih_l0"].shape == (4 * 64, 578)
    fresh = NativeOnPolicyRunner(envs[0], copy.deepcopy(cfgs[0]), log_dir=str(tmp_path / "resumed"), device="cuda:0")
    fresh.load(path)
    assert fresh.current_learning_iteration == 1
    envs[1].reset()          # (a runner resets its env when it is built: the uninterrupted run's env starts over with it)
    assert torch.equal(envs[0].obs_buf, envs[1].obs_buf) and torch.equal(envs[0].root_states, envs[1].root_states)
    _carry_over(fresh, runners[0])          # (runners[0] has lived what runners[1] has, bit for bit)
    fresh.learn(1)
    runners[1].learn(1)
    a, b = fresh.alg.optimizer_state(), runners[1].alg.optimizer_state()
    assert a["step"] == b["step"] and a["learning_rate"] == b["learning_rate"]
    for part in ("parameters", "exp_avg", "exp_avg_sq"):
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), (part, k, float((a[part][k] - b[part][k]).abs().max()))
    for e in envs:
        e.core.close()


def test_train_and_play_scripts_resume_the_recurrent_checkpoint(tmp_path, monkeypatch):
    """`scripts/train.py --runner native --sensor_collection native` on the raycast task with the recurrent policy and `empirical_normalization`, then
    `scripts/play.py --runner native`, which resumes what it saved."""
    import glob
    import os

    import extended_legged_gym_amd.utils.task_registry as tr
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.scripts.play import play
    from extended_legged_gym_amd.scripts.train import train
    from extended_legged_gym_amd.utils.helpers import get_args
    monkeypatch.setattr(tr, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    env_cfg, tcfg = task_registry.get_cfgs(TASK)
    keep = (copy.deepcopy(env_cfg), copy.deepcopy(tcfg))
    try:
        env_cfg.terrain.confined_terrain_proportions = ENV_OVER["terrain.confined_terrain_proportions"]
        env_cfg.terrain.num_rows, env_cfg.terrain.num_cols = 5, 5          # (what play.py sets: both scripts then build the same terrain)
        tcfg.runner.num_steps_per_env, tcfg.runner.save_interval = T, 1
        tcfg.runner.policy_class_name, tcfg.runner.empirical_normalization = "ActorCriticRecurrent", True
        if hasattr(tcfg.policy, "class_name"):
            tcfg.policy.class_name = "ActorCriticRecurrent"
        tcfg.policy.rnn_hidden_size, tcfg.policy.rnn_type, tcfg.policy.rnn_num_layers = 64, "lstm", 1
        common = ["--task", TASK, "--runner", "native", "--num_envs", str(N), "--experiment_name", "wide_recurrent_test"]
        train(get_args(common + ["--max_iterations", "1", "--sensor_collection", "native"]))
        runs = glob.glob(str(tmp_path / "logs" / "wide_recurrent_test" / "*"))
        assert len(runs) == 1 and "model_0.pt" in os.listdir(runs[0])
        ck = torch.load(os.path.join(runs[0], "model_0.pt"), map_location="cpu", weights_only=False)
        assert ck["model_state_dict"]["memory_a.rnn.weight_ih_l0"].shape == (4 * 64, 578) and "obs_norm_state_dict" in ck
        stats = play(get_args(common), num_steps=3)
        assert stats["steps"] == 3 and math.isfinite(stats["mean_reward"])
    finally:          # train / play and the argument overrides write into the registered instances: put pristine copies back
        task_registry.env_cfgs[TASK], task_registry.train_cfgs[TASK] = keep
