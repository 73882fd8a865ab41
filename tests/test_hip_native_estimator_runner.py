"""GPU: `rl.NativeTerrainEstimatorRunner` on `elspider_air_rough_raycast`: 8 envs, 8 steps per iteration, `gradient_length` 4, 3 iterations.

* loss parity: `learn` gives, bit for bit, the losses of the loop of `tools/train_estimator.py --collect one-call --update native` (its `make_env`,
  `collect_estimation(one_call=True)` and `NativeEstimatorDistillation.update`) from the same seed, initial weights and pre-drawn actions;
* resume: save after two iterations, a fresh runner on a fresh env brought to the same point, `load`, one more iteration: the parameters, both Adam
  moments, the step count and the loss of the uninterrupted run;
* the saved file loads into `TerrainEstimatorTorch` + `torch.optim.Adam` and holds the reference's four keys;
* pretrained policies: a two-iteration `NativeOnPolicyRunner` checkpoint with `empirical_normalization`, feed-forward and `ActorCriticRecurrent`,
  drives the one call (the host loop is not entered); a checkpoint with `obs_mean` / `obs_var` goes through the host loop;
* `play` returns the per-ray table and leaves the trained parameters alone; with `encoder_precision = "bf16"` it steps a bf16 estimator while
  training stayed fp32."""
import math
import os
import sys

import pytest
import torch

from tests.test_env_api import make
from tests.test_hip_estimator import ENV_OVER

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
TASK, N, T, G, SEED = "elspider_air_rough_raycast", 8, 8, 4, 4


def estimator_cfg(**runner):
    from extended_legged_gym_amd.scripts.terrain_est_train import create_terrain_estimator_config, get_terrain_estimator_args
    cfg = create_terrain_estimator_config(get_terrain_estimator_args(["--num_steps_per_env", str(T), "--gradient_length", str(G), "--num_learning_epochs", "1"]))
    cfg["algorithm"]["max_grad_norm"] = None          # the tool's loop clips nothing
    cfg["runner"].update(dict(sensor_collection="native"), **runner)
    cfg["seed"] = SEED
    return cfg


def tool_env():
    from train_estimator import make_env
    return make_env(N, SEED, small_terrain=True)


def _flat(state):
    return {k: (v if not isinstance(v, dict) else {n: t.clone() for n, t in v.items()}) for k, v in state.items()}


def _same_state(a, b):
    assert a["step"] == b["step"] and a["learning_rate"] == b["learning_rate"]
    for part in ("parameters", "exp_avg", "exp_avg_sq"):
        for name in a[part]:
            assert torch.equal(a[part][name], b[part][name]), (part, name)


def test_learn_gives_the_losses_of_the_tools_loop(tmp_path):
    from extended_legged_gym_amd.rl import NativeEstimatorDistillation, NativeTerrainEstimator, NativeTerrainEstimatorRunner, collect_estimation
    env = tool_env()
    runner = NativeTerrainEstimatorRunner(env, estimator_cfg(), log_dir=str(tmp_path), device="cuda:0")
    assert runner.one_call and runner.pretrained_policy is None
    runner.learn(3)
    assert runner.host_collections == 0 and runner.current_learning_iteration == 2
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pt")) == ["estimator_0.pt", "estimator_2.pt"]
    start, shape, R = runner.initial_state_dict, runner.depth_image_shape, runner.num_raycast_outputs
    # the tool's loop (tools/train_estimator.py, train(collect="one-call", update="native")) on a second env
    env2 = tool_env()
    env2.reset()          # (the runner's constructor resets its env, as the reference's does)
    trained = NativeTerrainEstimator(start, shape, 6, device="cuda:0")
    alg = NativeEstimatorDistillation(trained, start, gradient_length=G, learning_rate=1e-3)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    curve = []
    for _ in range(3):
        drawn = torch.randn(T, N, env2.num_actions, device="cuda", generator=gen) * 0.5
        with torch.inference_mode():
            rows = collect_estimation(env2, None, T, one_call=True, actions=drawn)
        curve.append(alg.update(rows)["estimation"])
    print("losses of learn:", runner.losses, " of the tool's loop:", curve)
    assert runner.losses == curve and all(math.isfinite(v) for v in curve)
    _same_state(runner.alg.optimizer_state(), alg.optimizer_state())
    # the scalars of the reference's log
    import json
    tags = {json.loads(line)["tag"] for line in open(tmp_path / "scalars.jsonl")} if (tmp_path / "scalars.jsonl").exists() else None
    if tags is not None:
        assert {"Loss/estimation", "Train/learning_rate", "Train/grad_norm", "Train/mean_estimation_loss", "Perf/total_fps", "Perf/collection_time",
                "Perf/learning_time"} <= tags
    for e in (env, env2):
        e.core.close()


def test_resume_and_interchange_with_torch(tmp_path):
    from extended_legged_gym_amd.rl import NativeTerrainEstimatorRunner, TerrainEstimatorTorch
    env = tool_env()
    a = NativeTerrainEstimatorRunner(env, estimator_cfg(save_interval=100), log_dir=str(tmp_path), device="cuda:0")
    a.learn(2)
    path = str(tmp_path / "estimator_1.pt")
    assert os.path.exists(path)
    saved_state = _flat(a.alg.optimizer_state())
    a.disable_logs = True
    a.learn(1)
    want_loss, want_state = a.losses[-1], a.alg.optimizer_state()
    # a fresh runner on a fresh env, brought to where the first one stood: two collections move the env and the action generator
    env2 = tool_env()
    b = NativeTerrainEstimatorRunner(env2, estimator_cfg(), log_dir=None, device="cuda:0")
    for _ in range(2):
        b._collect_rows(T)
    b.load(path)
    assert b.current_learning_iteration == 1
    _same_state(b.alg.optimizer_state(), saved_state)
    b.learn(1)
    print("next loss, uninterrupted:", want_loss, " resumed:", b.losses[-1])
    assert b.losses[-1] == want_loss
    _same_state(b.alg.optimizer_state(), want_state)
    # the file: the reference's four keys, loaded by the torch restatement and torch's Adam
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(ck) == ["infos", "iter", "model_state_dict", "optimizer_state_dict"] and ck["iter"] == 1
    model = TerrainEstimatorTorch(a.depth_image_shape, 6, a.num_raycast_outputs)
    model.load_state_dict(ck["model_state_dict"])
    opt = torch.optim.Adam(model.parameters(), lr=0.5)
    opt.load_state_dict(ck["optimizer_state_dict"])
    assert opt.param_groups[0]["lr"] == 1e-3
    for (name, p) in model.named_parameters():
        assert torch.equal(p.detach(), saved_state["parameters"][name]) and torch.equal(opt.state[p]["exp_avg"], saved_state["exp_avg"][name])
        assert float(opt.state[p]["step"]) == saved_state["step"] == 2 * (T // G)
    sum((p ** 2).sum() for p in model.parameters()).backward()
    opt.step()
    # and the other way round: what torch's Adam saves loads into the runner
    other = str(tmp_path / "from_torch.pt")
    torch.save({"model_state_dict": model.state_dict(), "optimizer_state_dict": opt.state_dict(), "iter": 7, "infos": None}, other)
    assert b.load(other) is None and b.current_learning_iteration == 7 and b.alg.optimizer_state()["step"] == saved_state["step"] + 1
    for e in (env, env2):
        e.core.close()


def _policy_checkpoint(tmp_path, policy_class_name):
    """Two iterations of `NativeOnPolicyRunner` with `empirical_normalization` on the task: `model_1.pt`."""
    from extended_legged_gym_amd.rl import NativeOnPolicyRunner
    from tests.test_hip_native_runner import train_cfg
    cfg = train_cfg(TASK, num_steps_per_env=4, empirical_normalization=True, sensor_collection="native", policy_class_name=policy_class_name)
    cfg["policy"].update(rnn_type="gru", rnn_hidden_size=24, rnn_num_layers=1)
    env = make(TASK, N, **ENV_OVER)
    log_dir = tmp_path / ("policy_" + policy_class_name)
    NativeOnPolicyRunner(env, cfg, log_dir=str(log_dir), device="cuda:0").learn(2)
    env.core.close()
    return str(log_dir / "model_1.pt"), cfg["policy"]


@pytest.mark.parametrize("policy_class_name", ["ActorCritic", "ActorCriticRecurrent"])
def test_runner_checkpoint_drives_the_one_call(tmp_path, policy_class_name, monkeypatch):
    from extended_legged_gym_amd.rl import NativeTerrainEstimatorRunner, estimator_runner
    path, policy_cfg = _policy_checkpoint(tmp_path, policy_class_name)
    assert "obs_norm_state_dict" in torch.load(path, map_location="cpu", weights_only=False)
    cfg = estimator_cfg(policy_class_name=policy_class_name)
    cfg["policy"] = dict(policy_cfg)
    env = tool_env()
    runner = NativeTerrainEstimatorRunner(env, cfg, pretrained_policy_path=path, device="cuda:0")
    assert runner.pretrained_policy is not None and runner.policy_normalizer is not None and not runner.policy_normalizer.training
    assert runner.pretrained_policy.is_recurrent == (policy_class_name == "ActorCriticRecurrent") and runner.policy_width == 578

    def no_host_loop(*a, **k):
        raise AssertionError("the host loop was entered")
    monkeypatch.setattr(estimator_runner, "collect_estimation", no_host_loop)
    count = runner.policy_normalizer.get_state()[3]
    runner.learn(1)
    assert runner.one_call and runner.host_collections == 0 and math.isfinite(runner.losses[0]) and runner.policy_normalizer.get_state()[3] == count
    env.core.close()


def test_obs_mean_checkpoint_goes_through_the_host_loop(tmp_path, capsys):
    from extended_legged_gym_amd.rl import NativeTerrainEstimatorRunner
    from extended_legged_gym_amd.rl.runner import initial_state_dict
    policy_cfg = dict(actor_hidden_dims=[32, 16], critic_hidden_dims=[24], activation="elu")
    sd = initial_state_dict("ActorCritic", 578, 18, policy_cfg, seed=3)
    path = str(tmp_path / "reference_style.pt")
    torch.save({"model_state_dict": sd, "obs_mean": torch.zeros(578), "obs_var": torch.ones(578)}, path)
    cfg = estimator_cfg()
    cfg["policy"] = policy_cfg
    env = tool_env()
    runner = NativeTerrainEstimatorRunner(env, cfg, pretrained_policy_path=path, device="cuda:0")
    assert not runner.one_call and "obs_mean" in runner.sensor_refusal
    runner.learn(1)
    assert runner.host_collections == 1 and math.isfinite(runner.losses[0])
    # a path that does not exist: the reference's warning, random actions
    capsys.readouterr()
    other = NativeTerrainEstimatorRunner(env, estimator_cfg(), pretrained_policy_path=str(tmp_path / "missing.pt"), device="cuda:0")
    assert "Warning: No pretrained policy provided. Environment will use random actions." in capsys.readouterr().out and other.pretrained_policy is None
    env.core.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_play_returns_the_per_ray_table(precision):
    from extended_legged_gym_amd.rl import NativeTerrainEstimatorRunner
    env = make(TASK, N, **ENV_OVER, **{"env.episode_length_s": 0.4})          # episodes of 20 steps: every env ends inside the third block of 8
    runner = NativeTerrainEstimatorRunner(env, estimator_cfg(play_block_steps=8, encoder_precision=precision), device="cuda:0")
    runner.learn(1)
    before = runner.alg.optimizer_state()
    table = runner.play(num_episodes=4)
    R = runner.num_raycast_outputs
    assert all(table[k].shape == (R,) and bool(torch.isfinite(table[k]).all()) for k in ("rmse", "mae", "bias", "max"))
    assert bool((table["max"] >= table["mae"]).all()) and bool((table["mae"] >= 0).all()) and bool((table["rmse"] >= table["mae"]).all())
    assert table["episodes"] >= 4 and table["steps"] % 8 == 0
    _same_state(runner.alg.optimizer_state(), before)
    assert runner._estimator_for_play().precision == precision and runner.estimator.precision == "fp32" and math.isfinite(runner.losses[0])
    assert runner.get_inference_estimator() is runner.estimator
    runner.close()
    env.core.close()
